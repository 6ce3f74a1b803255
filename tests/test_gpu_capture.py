"""GPU: every compute path replayed from a captured graph, against its eager launch.

A replay runs none of the Python or host C code again: only what was recorded as device work
survives. So every per-call decision must be made on the device (the fixed-point forward's
per-task fallback, ref_compat slot counts, the padding mask of the backward) and every piece of
per-call clean-up must be a node of the chain (the zeroing of split rows before the segment
atomics, the memsets of ``bwd_flush = 1``, of the forward's statistics words and of the fused
top-k's pair). No eager test can see a decision baked at capture or a clean-up that does not
replay; these tests can.

One protocol (:func:`replay_protocol`) for every case, on static tensors allocated before the
capture, everything on one side stream, so each graph is a plain chain of kernel and memset
nodes:

1. input set A, one eager call (plans, LDS attributes), synchronise;
2. capture the same call;
3. copy set B into the static inputs, fill every static output with a poison byte of
   ``arena.POISONS`` (or restore the prior of an accumulating output), replay;
4. compare with the reference and with the eager result of B computed into separate buffers;
5. replay again, touching nothing: bit-identical to 3 (missing zeroing, accumulation);
6. set C, which switches regime (wide range, non-finite, padding slots), replay, compare; then
   B again: the bits of 3 (the path returns from the fallback).

No new tolerance: the top-k family, the scatters, the SDDMM and ``cbsr_stats`` are bit-equal to
the oracle or numpy restatement the eager tests use; the forward and backward on B run exactly
summable data (integer features, edge values in {0.5, 1, 2}, dropout scale 2; the precondition
``structured.exactly_summable`` is asserted on the CPU), so replay, eager run and f64 oracle agree
bit for bit whatever the atomic order; on C they are held to ``oracle.close_enough`` at its
default bar / ``structured.assert_same_nonfinite_and_close``, as the eager structured tests are,
and the eager run of C passes the same bar in the same test. Against a vacuous pass the
references of A and B must differ in a large share of elements, and no poison may survive a
replay.

Edge values are a snapshot held by the plan: a replay computes with the values the plan held,
whatever the caller's tensor holds by then (test_values_are_a_snapshot). The three calls whose
host-side work a replay would skip are refused during capture (the last tests of the file).
"""
import functools
import time
import types

import numpy as np
import pytest
import torch

import maxk_kernels as mk
import structured as st
from arena import POISONS
from maxk_kernels import graphs, ops
from maxk_kernels.layers import MaxKGIN, MaxKSAGE
from oracle import oracle
from test_dropout_capi import drop_scale, dropped_table, keep_mask
from test_edge_grad_capi import edge_grad_rows
from test_gpu_contracts import stats_pair
from test_gpu_edge_grad import GRAPHS as EDGE_GRAPHS
from test_gpu_edge_grad import assert_same_bits, grads as edge_grads, tables as edge_tables
from test_gpu_parity import empty_rows_graph, graph_on, heavy_graph, to_dev
from test_gpu_records import chunk_bytes, pack_records
from test_gpu_self import _filled_count
from test_gpu_structured import block_cols, check_range_forward
from test_layers import close, small_edges
from test_self_capi import dense_rows, merge_rows

pytestmark = pytest.mark.gpu

SEED = 0x5EEDF00D12345678
TAGS = ("A", "B", "C")
COUNTS = {f: 0 for f in ("top-k", "scatter", "forward", "backward", "SDDMM", "dense", "autograd",
                         "refusals")}
T0 = time.time()
_STREAM = []


def side_stream():
    """The one stream everything here runs on: eager calls, captures and replays."""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


# =========================================================================== the protocol
def host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    diff = np.argwhere(raw(got) != raw(want))
    assert diff.size == 0, (f"{what}: {len(diff)} of {got.size} elements differ, first at "
                            f"{tuple(int(i) for i in diff[0])}: got {got[tuple(diff[0])]!r}, "
                            f"want {want[tuple(diff[0])]!r}")


def assert_bits_nan(got, want, what):
    """Bit-equal except that a NaN only has to be a NaN (payloads are unspecified)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert_same_bits(got.reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1), what)


def assert_equal_floats(got, ref, what):
    """Equal as floats to the f64 oracle rounded to f32 (test_gpu_structured's comparison)."""
    ref = np.asarray(ref).astype(np.float32)
    bad = got != ref
    assert got.shape == ref.shape and not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
        f"{tuple(int(i) for i in np.argwhere(bad)[0])}: got {got[bad][:4]}, oracle {ref[bad][:4]}")


def assert_differ(a, b, what):
    """The precondition against a vacuous pass: sets A and B ask for different results, in at
    least half of the elements that are not zero in both (a scatter's output is mostly zeros)."""
    ra = raw(np.asarray(a, np.float32) if a.dtype.kind == "f" else a)
    rb = raw(np.asarray(b, np.float32) if b.dtype.kind == "f" else b)
    live = (ra != 0) | (rb != 0)
    share = float((ra != rb)[live].mean()) if live.any() else 0.0
    assert live.mean() >= 0.01 and share >= 0.5, (
        f"{what}: the references of A and B differ in only {share:.2%} of their nonzero elements")


def poisoned(a, poison):
    """Elements of an f32 / i32 array whose every byte still holds the poison."""
    word = np.uint32(poison * 0x01010101)
    return int((raw(a) == word).sum()) if a.dtype.itemsize == 4 else 0


def replay_protocol(case, poison):
    """``case``: ``sets`` {tag: {name: numpy}} (the inputs A, B, C), ``outs()`` -> fresh
    caller-owned outputs {name: tensor}, ``call(i, o)`` -> every output {name: tensor},
    ``check(tag, got, eager)`` asserting one result ({name: numpy}; ``eager`` is the eager result
    of the same set when ``got`` is a replay), ``main``: the output whose references
    ``case.ref(tag)`` must differ between A and B, ``exact``: a replay of B is deterministic
    (bit-equal to the eager run and to every other replay); optional ``place`` {name: numpy ->
    tensor} (a strided input), ``prior`` {name: tensor} (contents an accumulating output is
    given before every call), ``trim`` {name: numpy -> numpy} (the part of an output the call
    defines: a record's bytes past its chunks are never written)."""
    s = side_stream()
    place = getattr(case, "place", {})
    prior = getattr(case, "prior", {})
    trim = getattr(case, "trim", {})

    def grab(res):
        return {n: trim[n](host(t)) if n in trim else host(t) for n, t in res.items()}

    def put(name, a):
        return place[name](a) if name in place else to_dev(a, DEV[0])

    with torch.cuda.stream(s):
        eager = {}
        for tag in TAGS:
            res = case.call({n: put(n, a) for n, a in case.sets[tag].items()}, case.outs())
            s.synchronize()
            eager[tag] = grab(res)
            case.check(tag, eager[tag], None)
        assert_differ(case.ref("A"), case.ref("B"), case.what)

        si = {n: put(n, a) for n, a in case.sets["A"].items()}
        so = case.outs()
        case.call(si, so)                                            # 1
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                          # 2
            res = case.call(si, so)

        def replay(tag=None):
            with torch.no_grad():
                if tag is not None:
                    for n, a in case.sets[tag].items():
                        si[n].copy_(to_dev(a, DEV[0]))
                    for n, t in res.items():
                        if n not in prior:
                            t.view(torch.uint8).fill_(poison)
                for n, t in prior.items():
                    res[n].copy_(t)
            g.replay()
            s.synchronize()
            got = grab(res)
            left = {n: poisoned(a, poison) for n, a in got.items()}
            assert not any(left.values()), f"{case.what}: poison left after replay: {left}"
            return got

        def same(a, b, what):
            for n in a:
                assert same_bits(a[n], b[n]), f"{case.what}: {n}: {what}"

        b1 = replay("B")                                             # 3
        case.check("B", b1, eager["B"])                              # 4
        if case.exact:
            same(b1, eager["B"], "replay of B differs from the eager run of B")
        b2 = replay()                                                # 5
        if case.exact:
            same(b2, b1, "a second replay changed the output")
        else:
            case.check("B", b2, eager["B"])
        case.check("C", replay("C"), eager["C"])                     # 6
        b3 = replay("B")
        if case.exact:
            same(b3, b1, "B after C differs from B before C")
        else:
            case.check("B", b3, eager["B"])
    del g
    COUNTS[case.family] += 1


DEV = []


@pytest.fixture(autouse=True)
def _device(gpu):
    DEV[:] = [gpu]
    yield
    torch.cuda.synchronize()


def case_of(family, what, **kw):
    return types.SimpleNamespace(family=family, what=what, **kw)


# =========================================================================== inputs
@functools.lru_cache(maxsize=None)
def exact_graph(name):
    """The structure of ``heavy_graph()`` (two rows split into segments) or ``empty_rows_graph()``
    with edge values drawn from {0.5, 1, 2}."""
    p, ix, _ = heavy_graph() if name == "heavy" else empty_rows_graph()
    rs = np.random.RandomState(9)
    return p, ix, rs.choice(np.array([0.5, 1.0, 2.0], np.float32), ix.size).astype(np.float32)


def wide_rows(x):
    """The odd rows scaled by 2^-60: past what one fixed-point scale holds."""
    x = x.copy()
    x[1::2] *= np.float32(2.0 ** -60)
    return x


def nonfinite_rows(x):
    x = x.copy()
    x[0, 7], x[1, 9], x[2, 11] = np.inf, -np.inf, np.nan
    return x


@functools.lru_cache(maxsize=8)
def feature_sets(n, d, k, kind):
    """Integer features A and B, and C: B with wide-range rows or with non-finite entries."""
    a = st.int_features(n, d, seed=4100 + k)
    b = st.int_features(n, d, seed=4200 + k)
    return {"A": a, "B": b, "C": wide_rows(b) if kind == "range" else nonfinite_rows(b)}


def compare_sum(got, ref, mag, tag, what):
    """A forward / backward output: exact sets equal the oracle as floats, C is at the eager
    structured tests' bars."""
    if tag in ("A", "B"):
        assert st.exactly_summable(mag), f"{what}: set {tag} is not exactly summable"
        assert_equal_floats(got, ref, f"{what} set {tag}")
    else:
        try:
            st.assert_same_nonfinite_and_close(got, ref, mag)
        except AssertionError as exc:
            raise AssertionError(f"{what} set C: {exc}") from None


# =========================================================================== top-k
TOPK_OPTIONS = ["plain", "stats", "rec2", "rec4", "rec1", "dense", "dropout", "all"]


def topk_sets(n, d, mode):
    a = graphs.features(n, d, seed=300 + n + d).numpy()
    b = graphs.features(n, d, seed=301 + n + d).numpy().copy()
    if mode == "ref_compat":
        b[::3, 5] = 1e6                        # single-hit rows: padding slots A did not have
    c = nonfinite_rows(graphs.features(n, d, seed=302 + n + d).numpy())
    c[3] = 0.0                                 # constant rows: ref_compat fills no slot
    c[4] = 2.5
    return {"A": {"x": a}, "B": {"x": b}, "C": {"x": c}}


@functools.lru_cache(maxsize=None)
def topk_ref(n, d, k, mode, p, tag):
    x = topk_sets(n, d, mode)[tag]["x"]
    od, oi = oracle.maxk(x, k, mode)
    cnt = (np.full(n, k) if mode == "exact" else _filled_count(od, oi)).astype(np.int32)
    val = dropped_table(od, oi, p, SEED) if p else od
    return types.SimpleNamespace(values=val, index=oi, count=cnt,
                                 dense=dense_rows(val, oi, cnt, d))


@pytest.mark.parametrize("option", TOPK_OPTIONS)
@pytest.mark.parametrize("n,d", [(5, 256), (1000, 256), (5, 100), (1000, 100)])
@pytest.mark.parametrize("mode", ["exact", "ref_compat"])
def test_capture_topk(gpu, mode, n, d, option):
    """``ops.maxk_forward`` in both modes: the plain launch, with ``stats=`` (a memset and two
    launches), ``records=`` of layouts 2, 4 and 1, ``dense=``, ``dropout=`` and all of them at
    once. B in ref_compat mode has single-hit rows, C rows with NaN and +-Inf and constant rows
    (count 0). With dropout the replayed table is ``dropped_table`` of the seed baked at capture:
    the documented meaning of an explicit seed, a replay draws no new mask."""
    k = {"rec2": 8, "rec4": 16, "rec1": 16}.get(option, 16 if d == 256 else 10)
    layout = {"rec2": 2, "rec4": 4, "rec1": 1, "all": 4}.get(option, 0)
    p = 0.5 if option in ("dropout", "all") else 0.0
    used = chunk_bytes(layout, k) if layout else 0
    rb = (used + 15) // 16 * 16 + 16
    has_stats, has_dense = option in ("stats", "all"), option in ("dense", "all")

    def outs():
        o = {"values": torch.empty((n, k), device=gpu),
             "index": torch.empty((n, k), dtype=torch.uint8, device=gpu)}
        if has_stats:
            o["stats"] = torch.empty(2, dtype=torch.int32, device=gpu)
        if layout:
            o["records"] = torch.empty((n, rb), dtype=torch.uint8, device=gpu)
        if has_dense:
            o["dense"] = torch.empty((n, d), device=gpu)
        return o

    def call(i, o):
        res = ops.maxk_forward(i["x"], k, mode=mode, return_index=True,
                               out=(o["values"], o["index"]), return_count=mode != "exact",
                               stats=o.get("stats"),
                               records=(o["records"], layout) if layout else None,
                               dropout=(p, SEED) if p else None, dense=o.get("dense"))
        return dict(o, count=res[2]) if mode != "exact" else dict(o)

    what = f"top-k {mode} N={n} D={d} k={k} {option}"

    def check(tag, got, eager):
        r = topk_ref(n, d, k, mode, p, tag)
        assert_bits(got["index"], r.index, f"{what} {tag} index")
        assert_bits(got["values"], r.values, f"{what} {tag} values")
        if mode != "exact":
            assert_bits(got["count"], r.count, f"{what} {tag} count")
        if has_dense:
            assert_bits(got["dense"], r.dense, f"{what} {tag} dense")
        if layout:
            want = pack_records(torch.from_numpy(r.values), torch.from_numpy(r.index), layout, rb)
            assert_bits(got["records"][:, :used], want.numpy()[:, :used], f"{what} {tag} records")
        if has_stats:
            if tag != "C":                     # finite tables: bit order is magnitude order
                assert_bits(got["stats"], stats_pair(r.values), f"{what} {tag} stats")
            elif eager is not None:            # the eager tests pin these to maxk_cbsr_stats
                assert_bits(got["stats"], eager["stats"], f"{what} {tag} stats")

    if mode == "ref_compat":
        ca, cb = (topk_ref(n, d, k, mode, p, t).count for t in "AB")
        assert (cb[::3] == 1).all() and (ca[::3] > 1).all()
        assert (topk_ref(n, d, k, mode, p, "C").count[3:5] == 0).all()
    replay_protocol(case_of("top-k", what, sets=topk_sets(n, d, mode), outs=outs, call=call,
                            check=check, exact=True, main="values",
                            trim={"records": lambda a: a[:, :used]},
                            ref=lambda tag: topk_ref(n, d, k, mode, p, tag).values),
                    POISONS[(n + d + k) % 2])


# =========================================================================== scatters
@pytest.mark.parametrize("option", ["plain", "strided", "dropout", "merge", "merge_dropout"])
@pytest.mark.parametrize("n,d,k", [(5, 256, 16), (1000, 256, 16), (1000, 100, 10)])
def test_capture_scatter(gpu, n, d, k, option):
    """``ops.maxk_backward`` with ``dim_origin``: plain, row-strided selectors, dropout, and the
    merge with ``grad_dense``. C: ref_compat selectors with padding slots (repeated feature 0,
    last slot wins) and NaN / +-Inf gradients."""
    p = 0.5 if "dropout" in option else 0.0
    merge = option.startswith("merge")
    sets = {}
    for j, tag in enumerate(TAGS):
        x = graphs.features(n, d, seed=500 + 3 * n + j).numpy().copy()
        if tag == "C":
            x[::3, 5] = 1e6
        _, oi = oracle.maxk(x, k, "ref_compat" if tag == "C" else "exact")
        gs = graphs.features(n, k, seed=510 + j).numpy().copy()
        gd = graphs.features(n, d, seed=520 + j).numpy().copy()
        if tag == "C":
            gs[0, 1], gs[1, 2], gs[2, 3] = np.nan, np.inf, -np.inf
            gd[1, int(oi[1, 2])], gd[2, 0] = -np.inf, np.nan
        sets[tag] = dict(gs=gs, si=oi, **({"gd": gd} if merge else {}))

    def strided(a):
        buf = torch.full((n, k + 5), 0xA5, dtype=torch.uint8, device=gpu)
        buf[:, :k] = to_dev(a, gpu)
        return buf[:, :k]

    def call(i, o):
        return {"gx": ops.maxk_backward(i["gs"], i["si"], dim_origin=d,
                                        dropout=(p, SEED) if p else None,
                                        grad_dense=i.get("gd"))}

    what = f"scatter N={n} D={d} k={k} {option}"

    @functools.lru_cache(maxsize=None)
    def ref(tag):
        z = sets[tag]
        if not merge and not p:
            return oracle.maxk_backward(z["gs"], z["si"], d)
        return merge_rows(z["gs"], z["si"], z.get("gd"), p, SEED, D=d)

    def check(tag, got, eager):
        assert_bits_nan(got["gx"], ref(tag), f"{what} {tag}")

    replay_protocol(case_of("scatter", what, sets=sets, outs=dict, call=call, check=check,
                            exact=True, main="gx", ref=ref,
                            place={"si": strided} if option == "strided" else {}),
                    POISONS[(n + k) % 2])


# =========================================================================== forward
@functools.lru_cache(maxsize=None)
def forward_ref(gname, k, kind, tag):
    """Tables and f64-oracle forward of one set on ``exact_graph(gname)``."""
    p, ix, v = exact_graph(gname)
    x = feature_sets(p.size - 1, 256, k, kind)[tag]
    od, oi = oracle.maxk(x, k)
    ref, mag = oracle.spgemm_forward(p, ix, v, od, oi, 256, with_mag=True)
    return types.SimpleNamespace(x=x, od=od, oi=oi, ref=ref, mag=mag)


# (graph, k, plan options, expected fwd_layout, expected fwd_fixed, form, C)
FWD_CASES = [
    ("heavy", 16, {}, 4, 1, "tables", "range"),          # pair-chunk pack + statistics pass
    ("heavy", 16, {}, 4, 1, "tables", "nonfinite"),
    ("empty", 16, {}, 4, 1, "tables", "nonfinite"),
    ("heavy", 8, {}, 2, 0, "tables", "range"),           # lane chunks
    ("empty", 8, {}, 2, 0, "tables", "nonfinite"),
    ("heavy", 32, {}, 0, 1, "tables", "range"),          # two tables
    ("empty", 32, {}, 0, 1, "tables", "nonfinite"),
    ("heavy", 7, dict(fwd_chunk3=2), 3, 0, "tables", "nonfinite"),
    ("empty", 7, dict(fwd_chunk3=2), 3, 0, "tables", "range"),
    ("heavy", 16, dict(fwd_fixed=1), 4, 1, "tables", "range"),
    ("empty", 16, dict(fwd_fixed=1), 4, 1, "tables", "nonfinite"),
    ("heavy", 16, dict(fwd_fixed=2), 4, 0, "tables", "range"),
    ("empty", 16, dict(fwd_fixed=2), 4, 0, "tables", "nonfinite"),
    ("heavy", 16, {}, 4, 1, "accumulate", "range"),
    ("empty", 16, {}, 4, 1, "accumulate", "nonfinite"),
    ("heavy", 16, {}, 4, 1, "records", "range"),         # the top-k writes the records
    ("heavy", 8, {}, 2, 0, "records", "nonfinite"),
    ("empty", 16, dict(fwd_chunk3=2, fwd_two_tables=2), 1, 1, "records", "range"),
]


@pytest.mark.parametrize("gname,k,opts,layout,fixed,form,kind", FWD_CASES,
                         ids=lambda v: ",".join(f"{a}={b}" for a, b in v.items()) or "default"
                         if isinstance(v, dict) else str(v))
def test_capture_forward(gpu, gname, k, opts, layout, fixed, form, kind):
    """``GraphPlan.forward`` / ``forward_records``. On ``heavy_graph`` two rows are split into
    segments added with atomics into rows a ``zero_rows`` launch (or the statistics pass) zeroes:
    if that did not replay, the second replay would double them. C forces the per-call f64
    fallback from the data alone: rows of the table 2^-60 apart, or NaN / +-Inf entries.
    ``accumulate``: ``out`` gets its prior back before every replay. ``records``: the top-k that
    writes the records (and the statistics pair a fixed-point forward reads) is captured in the
    same graph."""
    p, ix, v = exact_graph(gname)
    n, d = p.size - 1, 256
    ptr, idx, val = graph_on(gpu, p, ix, v)
    plan = mk.GraphPlan(ptr, idx, val, n, ix.size, d, k, options=opts)
    info = plan.info()
    assert (info["fwd_layout"], info["fwd_fixed"]) == (layout, fixed), info
    assert info["fwd_split_rows"] == (2 if gname == "heavy" else 0)
    what = f"forward {gname} k={k} {opts} {form} C={kind}"
    refs = functools.partial(forward_ref, gname, k, kind)
    acc = form == "accumulate"
    prior_np = st.int_features(n, d, seed=77) if acc else None
    prior = {"out": to_dev(prior_np, gpu)} if acc else {}
    if kind == "nonfinite":
        assert not np.isfinite(refs("C").ref).all()
    else:
        assert np.abs(refs("C").od[1::2]).max() < 2.0 ** -55

    def check_out(tag, got):
        r = refs(tag)
        ref, mag = (r.ref.astype(np.float64) + prior_np, r.mag + np.abs(prior_np)) if acc \
            else (r.ref, r.mag)
        compare_sum(got["out"], ref, mag, tag, what)

    if form == "records":
        rec_bytes = info["fwd_record_bytes"]
        used = chunk_bytes(layout, k)
        sets = {t: {"x": refs(t).x} for t in TAGS}

        def outs():
            o = {"out": torch.empty((n, d), device=gpu),
                 "records": torch.empty((n, rec_bytes), dtype=torch.uint8, device=gpu)}
            if fixed:
                o["stats"] = torch.empty(2, dtype=torch.int32, device=gpu)
            return o

        def call(i, o):
            st_ = o.get("stats")
            res = ops.maxk_forward(i["x"], k, return_index=True, records=(o["records"], layout),
                                   return_values=False, stats=st_)
            plan.forward_records(o["records"], layout, out=o["out"],
                                 stats=st_.view(1, 2) if st_ is not None else None)
            return dict(o, index=res[1])

        def check(tag, got, eager):
            r = refs(tag)
            assert_bits(got["index"], r.oi, f"{what} {tag} index")
            want = pack_records(torch.from_numpy(r.od), torch.from_numpy(r.oi), layout, rec_bytes)
            assert_bits(got["records"][:, :used], want.numpy()[:, :used], f"{what} {tag} records")
            if fixed and (tag != "C" or kind == "range"):
                assert_bits(got["stats"], stats_pair(r.od), f"{what} {tag} stats")
            check_out(tag, got)
    else:
        sets = {t: {"sd": refs(t).od, "si": refs(t).oi} for t in TAGS}

        def outs():
            return {"out": prior["out"].clone() if acc else torch.empty((n, d), device=gpu)}

        def call(i, o):
            plan.forward(i["sd"], i["si"], out=o["out"], accumulate=acc)
            return dict(o)

        def check(tag, got, eager):
            check_out(tag, got)

    replay_protocol(case_of("forward", what, sets=sets, outs=outs, call=call, check=check,
                            exact=True, main="out", ref=lambda tag: refs(tag).ref, prior=prior,
                            trim={"records": lambda a: a[:, :chunk_bytes(layout, k)]}
                            if form == "records" else {}),
                    POISONS[(k + len(form)) % 2])


@pytest.mark.parametrize("layout", [dict(), dict(fwd_chunk3=1)],
                         ids=["pair_chunks", "lane_chunks"])
@pytest.mark.parametrize("e", [24, 60, 100])
def test_capture_forward_range_tables(gpu, layout, e):
    """``structured.range_values("columns", e)``: a table whose rows span 2^e, replayed through a
    graph captured on the benign table of ``structured.range_tables``: the fixed-point forward
    must take the f64 fallback from the replayed statistics, and leave it again on B. The edge
    values are U(1, 2), not exactly summable, so every set is held to the eager test's bars
    (``test_gpu_structured.check_range_forward``) and replays are compared at those bars."""
    p, ix, _ = st.range_graph()
    val, data = st.range_values("benign")
    _, sel = st.range_tables()
    ptr, idx, dval = graph_on(gpu, p, ix, val)
    plan = mk.GraphPlan(ptr, idx, dval, st.RANGE_N, ix.size, st.RANGE_D, st.RANGE_K,
                        options=dict(layout, fwd_fixed=1, fwd_tile_rows=st.RANGE_TILE))
    assert plan.info()["fwd_fixed"] == 1 and plan.info()["fwd_split_rows"] == 0
    tables = {"A": data, "B": np.ascontiguousarray(-data[::-1]),
              "C": st.range_values("columns", e)[1]}
    sets = {t: {"sd": tables[t]} for t in TAGS}
    dsel = to_dev(sel, gpu)
    what = f"forward range columns e={e} {layout}"

    def call(i, o):
        plan.forward(i["sd"], dsel, out=o["out"])
        return dict(o)

    def check(tag, got, eager):
        check_range_forward(torch.from_numpy(got["out"]), val, tables[tag], f"{what} {tag}")

    def ref(tag):
        return oracle.spgemm_forward(p, ix, val, tables[tag], sel, st.RANGE_D)

    replay_protocol(case_of("forward", what, sets=sets, call=call, check=check, exact=False,
                            outs=lambda: {"out": torch.empty((st.RANGE_N, st.RANGE_D), device=gpu)},
                            main="out", ref=ref), POISONS[e % 2])


# =========================================================================== backward
@functools.lru_cache(maxsize=None)
def backward_ref(gname, k, tag):
    """Selectors, gradient and f64-oracle backward of one set on ``exact_graph(gname)``; C is
    B's with a NaN at feature 0 (which padded slots gather) and Infs at selected features."""
    p, ix, v = exact_graph(gname)
    n, d = p.size - 1, 256
    base = "B" if tag == "C" else tag
    _, oi = oracle.maxk(st.int_features(n, d, seed=4300 + k + ord(base)), k)
    g = st.int_features(n, d, seed=4400 + k + ord(base))
    if tag == "C":
        g = g.copy()
        rows = np.flatnonzero(np.diff(p) >= 2)[[3, 40, 400]]
        g[rows[0], 0] = np.nan
        g[rows[1], int(oi[ix[p[rows[1]]], min(3, k - 1)])] = np.inf
        g[rows[2], int(oi[ix[p[rows[2]] + 1], 0])] = -np.inf
    ref, mag = oracle.sspmm_backward(p, ix, v, g, oi, with_mag=True)
    return types.SimpleNamespace(g=g, oi=oi, ref=ref, mag=mag)


PIECES = dict(bwd_algo=1, bwd_piece_edges=2000)       # column blocks cut over work-groups
BWD_CASES = [
    ("heavy", 16, dict(PIECES, bwd_flush=2), "slabs"),
    ("empty", 16, dict(PIECES, bwd_flush=2), "slabs"),
    ("heavy", 16, dict(PIECES, bwd_flush=1), "atomics"),
    ("empty", 16, dict(PIECES, bwd_flush=1), "atomics"),
    ("heavy", 16, dict(PIECES, bwd_slot_groups=2), "groups"),
    ("heavy", 16, dict(bwd_algo=3), "two_pass"),
    ("empty", 16, dict(bwd_algo=3), "two_pass"),
    ("heavy", 7, dict(PIECES), "padded"),
    ("empty", 7, {}, "padded"),
    ("heavy", 16, {}, "default"),
]


@pytest.mark.parametrize("gname,k,opts,form", BWD_CASES,
                         ids=[f"{g}-k{k}-{f}" for g, k, _, f in BWD_CASES])
def test_capture_backward(gpu, gname, k, opts, form):
    """``GraphPlan.backward``: column blocks split over work-groups under ``bwd_flush`` 2 (slab
    combine, its slabs in the per-call workspace) and 1 (a memset of ``grad_sp``, then atomics:
    a replay without the memset would accumulate), two slot groups, the two-pass form with its
    E x k workspace taken from the allocator inside the capture, and k = 7 (padded slots)."""
    p, ix, v = exact_graph(gname)
    n, d = p.size - 1, 256
    ptr, idx, val = graph_on(gpu, p, ix, v)
    plan = mk.GraphPlan(ptr, idx, val, n, ix.size, d, k, options=opts)
    info = plan.info()
    assert info["bwd_algo"] == (3 if form == "two_pass" else 1), info
    if "bwd_piece_edges" in opts:
        assert info["bwd_shared_blocks"] > 0, info
    if form in ("slabs", "two_pass"):
        assert plan.bwd_ws_bytes > 0
    if form == "groups":
        assert info["bwd_block_cols"] == block_cols(n, 8), info
    what = f"backward {gname} k={k} {opts}"
    refs = functools.partial(backward_ref, gname, k)
    assert not np.isfinite(refs("C").ref).all()
    sets = {t: {"g": refs(t).g, "si": refs(t).oi} for t in TAGS}

    def call(i, o):
        plan.backward(i["g"], i["si"], grad_sp=o["gs"])
        return dict(o)

    def check(tag, got, eager):
        compare_sum(got["gs"], refs(tag).ref, refs(tag).mag, tag, what)

    replay_protocol(case_of("backward", what, sets=sets, call=call, check=check, exact=True,
                            outs=lambda: {"gs": torch.empty((n, k), device=gpu)},
                            main="gs", ref=lambda tag: refs(tag).ref), POISONS[len(form) % 2])


@pytest.mark.parametrize("case,k", [(c, 16) for c in st.NONFINITE_BWD] +
                         [("g_nan_f0", 7), ("g_inf_selected", 7)])
def test_capture_backward_nonfinite_cases(gpu, case, k):
    """``structured.NONFINITE_BWD`` as set C of a graph captured on finite gradients: a NaN or
    Inf appears in exactly the slots whose IEEE sum contains it. The graph's values are
    +-U(0.5, 1) (and those of the case, which the plan snapshots), so nothing is exactly
    summable: every set and every replay is held to ``assert_same_nonfinite_and_close``."""
    c = st.nonfinite_case(k, case)
    ptr, idx, val = graph_on(gpu, c.p, c.ix, c.v)
    plan = mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, c.d, k,
                        options=dict(bwd_algo=1) if k == 7 else dict(bwd_algo=3))
    gsets = {"A": graphs.features(c.n, c.d, seed=71).numpy(),
             "B": graphs.features(c.n, c.d, seed=72).numpy(), "C": c.g}
    sets = {t: {"g": gsets[t]} for t in TAGS}
    oi = to_dev(c.oi, gpu)
    what = f"backward nonfinite {case} k={k}"

    @functools.lru_cache(maxsize=None)
    def ref(tag):
        return oracle.sspmm_backward(c.p, c.ix, c.v, gsets[tag], c.oi, with_mag=True)

    def call(i, o):
        plan.backward(i["g"], oi, grad_sp=o["gs"])
        return dict(o)

    def check(tag, got, eager):
        try:
            st.assert_same_nonfinite_and_close(got["gs"], *ref(tag))
        except AssertionError as exc:
            raise AssertionError(f"{what} {tag}: {exc}") from None

    replay_protocol(case_of("backward", what, sets=sets, call=call, check=check, exact=False,
                            outs=lambda: {"gs": torch.empty((c.n, k), device=gpu)},
                            main="gs", ref=lambda tag: ref(tag)[0]), POISONS[k % 2])


# =========================================================================== other entry points
@pytest.mark.parametrize("name", ["straddle", "hub_row"])
def test_capture_edge_grad(gpu, name):
    """``ops.spgemm_edge_grad`` bit-equal to ``edge_grad_rows``; C: values over 2^+-60 with NaN
    and Inf entries."""
    p, ix, nc = EDGE_GRAPHS[name]
    n, d, k = p.size - 1, 64, 16
    ptr, idx = to_dev(p, gpu), to_dev(ix, gpu)
    sets = {}
    for j, tag in enumerate(TAGS):
        rng = np.random.default_rng(900 + j)
        values = "wide" if tag == "C" else "normal"
        v, sel = edge_tables(nc, k, d, rng, values=values)
        G = edge_grads(n, d, rng, values=values)
        if tag == "C":
            v[0, 1], v[1, 2], G[1, 3], G[2, 5] = np.nan, np.inf, -np.inf, np.nan
        sets[tag] = {"G": G, "v": v, "sel": sel}
    what = f"edge_grad {name}"

    def call(i, o):
        ops.spgemm_edge_grad(ptr, idx, i["G"], i["v"], i["sel"], n, ix.size, k, d, out=o["gv"])
        return dict(o)

    @functools.lru_cache(maxsize=None)
    def ref(tag):
        z = sets[tag]
        return edge_grad_rows(p, ix, z["G"], z["v"], z["sel"])

    def check(tag, got, eager):
        assert_same_bits(got["gv"], ref(tag), f"{what} {tag}")

    assert np.isnan(ref("C")).any()
    replay_protocol(case_of("SDDMM", what, sets=sets, call=call, check=check, exact=True,
                            outs=lambda: {"gv": torch.empty(ix.size, device=gpu)},
                            main="gv", ref=ref), POISONS[len(name) % 2])


@pytest.mark.parametrize("d", [64, 66])
def test_capture_dense_spmm(gpu, d):
    """``ops.dense_spmm`` at D = 64 and at a width that pads (66 -> 68 on a padded copy made
    inside the capture). C: rows 2^-40 apart, at the eager test's bar."""
    p, ix, v = exact_graph("empty")
    n = p.size - 1
    ptr, idx, val = graph_on(gpu, p, ix, v)
    a, b = st.int_features(n, d, seed=61), st.int_features(n, d, seed=62)
    c = b.copy()
    c[1::2] *= np.float32(2.0 ** -40)
    sets = {"A": {"x": a}, "B": {"x": b}, "C": {"x": c}}
    what = f"dense_spmm D={d}"

    @functools.lru_cache(maxsize=None)
    def ref(tag):
        x = sets[tag]["x"]
        return oracle.dense_spmm(p, ix, v, x), oracle.dense_spmm(p, ix, np.abs(v), np.abs(x))

    def check(tag, got, eager):
        out, mag = ref(tag)
        if tag == "C":
            ok, worst = oracle.close_enough(got["y"], out, mag, rtol=2e-6 * 64)
            assert ok, f"{what} C: worst err/bound {worst:.3g}"
        else:
            assert st.exactly_summable(mag)
            assert_equal_floats(got["y"], out, f"{what} {tag}")

    replay_protocol(case_of("dense", what, sets=sets, outs=dict, check=check, exact=True,
                            call=lambda i, o: {"y": ops.dense_spmm(ptr, idx, val, i["x"])},
                            main="y", ref=lambda tag: ref(tag)[0]), POISONS[d % 2])


@pytest.mark.parametrize("n,k", [(5, 16), (1000, 16), (1000, 10)])
def test_capture_cbsr_stats(gpu, n, k):
    """``ops.cbsr_stats`` (a memset of the pair, then the pass) bit-equal to ``stats_pair``; C: a
    ref_compat table with padding slots."""
    sets = {}
    for j, tag in enumerate(TAGS):
        x = graphs.features(n, 100, seed=40 + j).numpy().copy() * np.float32(3.0 ** j)
        if tag == "C":
            x[::3, 5] = 1e6
        od, oi = oracle.maxk(x, k, "ref_compat" if tag == "C" else "exact")
        sets[tag] = {"sd": od, "si": oi}
    what = f"cbsr_stats N={n} k={k}"

    def call(i, o):
        ops.cbsr_stats(i["sd"], i["si"], out=o["stats"])
        return dict(o)

    def check(tag, got, eager):
        assert_bits(got["stats"].reshape(-1), stats_pair(sets[tag]["sd"]), f"{what} {tag}")

    assert not np.array_equal(stats_pair(sets["A"]["sd"]), stats_pair(sets["B"]["sd"]))
    replay_protocol(case_of("dense", what, sets=sets, call=call, check=check, exact=True,
                            outs=lambda: {"stats": torch.empty((1, 2), dtype=torch.int32,
                                                               device=gpu)},
                            main="stats", ref=lambda tag: sets[tag]["sd"]), POISONS[n % 2])


# =========================================================================== whole steps
@functools.lru_cache(maxsize=None)
def step_ref(gname, k, mode, p, self_term, tag):
    """Inputs and f64-oracle results of one autograd step on ``exact_graph(gname)`` (the
    formulas of ``structured.exact_case``; with the self term the dense output's gradient is
    added at the selected features before the dropout factor)."""
    pp, ix, v = exact_graph(gname)
    n, d = pp.size - 1, 256
    x = st.int_features(n, d, seed=4500 + k + ord(tag[0])).copy()
    if tag != "A":
        x[::5, 9] = 64.0                       # ref_compat: rows with padding slots
    if tag == "C":
        x = wide_rows(x)
        x[3, 9] = np.inf
    g = st.int_features(n, d, seed=4600 + k + ord(tag[0]))
    gself = st.int_features(n, d, seed=4700 + k + ord(tag[0]))
    od0, oi = oracle.maxk(x, k, mode)
    od = dropped_table(od0, oi, p, SEED) if p else od0
    fwd, fwd_mag = oracle.spgemm_forward(pp, ix, v, od, oi, d, with_mag=True)
    bwd, bwd_mag = oracle.sspmm_backward(pp, ix, v, g, oi, with_mag=True)
    filled = od0 != 0 if mode == "ref_compat" else np.ones_like(od0, bool)
    count = filled.sum(1)
    scale = float(drop_scale(p)) if p else 1.0
    keep = keep_mask(p, SEED, np.arange(n)[:, None], oi) if p else np.ones_like(od0, bool)
    rows = np.repeat(np.arange(n)[:, None], k, 1)
    gsel = gself[rows, oi].astype(np.float64) if self_term else 0.0
    gx = np.zeros((n, d), np.float64)
    gx_mag = np.zeros((n, d), np.float64)
    gx[rows[filled], oi[filled]] = ((bwd.astype(np.float64) + gsel) * keep * scale)[filled]
    gx_mag[rows[filled], oi[filled]] = ((bwd_mag.astype(np.float64) + np.abs(gsel)) * scale)[filled]
    xm = dense_rows(od, oi, count, d) if self_term else None
    return types.SimpleNamespace(x=x, g=g, gself=gself, fwd=fwd, fwd_mag=fwd_mag, gx=gx,
                                 gx_mag=gx_mag, xm=xm, count=count)


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["plain", "dropout"])
@pytest.mark.parametrize("mode", ["exact", "ref_compat"])
@pytest.mark.parametrize("self_term", [False, True], ids=["aggregate", "self_aggregate"])
@pytest.mark.parametrize("gname,k", [("heavy", 16), ("empty", 32)])
def test_capture_autograd_step(gpu, gname, k, self_term, mode, p):
    """``maxk_aggregate`` / ``maxk_self_aggregate``, forward and backward in one captured graph
    (torch's whole-step pattern: static ``x`` with ``requires_grad``, a static upstream gradient,
    ``x.grad = None`` before every step so the backward writes it afresh): ``x.grad`` and the
    outputs after replay on B are bit-equal to an eager step on B and equal the oracle. In
    ref_compat mode B has rows with fewer than k filled slots that A did not have, so the slot
    counts and the padding mask of the backward must follow the replayed data. The dropout seed
    is explicit: the mask of capture time, on every replay."""
    pp, ix, v = exact_graph(gname)
    n, d = pp.size - 1, 256
    graph = mk.CSRGraph(*graph_on(gpu, pp, ix, v))
    refs = functools.partial(step_ref, gname, k, mode, p, self_term)
    what = f"autograd {gname} k={k} {mode} p={p} self={self_term}"
    if mode == "ref_compat":
        assert (refs("A").count == k).all() and (refs("B").count < k).sum() >= 50
    names = ("x", "g", "gself") if self_term else ("x", "g")
    sets = {t: {nm: getattr(refs(t), nm) for nm in names} for t in TAGS}

    def call(i, o):
        x = i["x"].requires_grad_(True)
        x.grad = None
        if self_term:
            xm, y = mk.maxk_self_aggregate(x, graph, k, mode, dropout_p=p, seed=SEED)
            torch.autograd.backward([xm, y], [i["gself"], i["g"]])
            return {"y": y.detach(), "xm": xm.detach(), "gx": x.grad}
        y = mk.maxk_aggregate(x, graph, k, mode, dropout_p=p, seed=SEED)
        torch.autograd.backward([y], [i["g"]])
        return {"y": y.detach(), "gx": x.grad}

    def check(tag, got, eager):
        r = refs(tag)
        compare_sum(got["y"], r.fwd, r.fwd_mag, tag, what + " y")
        compare_sum(got["gx"], r.gx, r.gx_mag, tag, what + " x.grad")
        if self_term:
            assert_bits(got["xm"], r.xm, f"{what} {tag} x_masked")

    replay_protocol(case_of("autograd", what, sets=sets, outs=dict, call=call, check=check,
                            exact=True, main="gx", ref=lambda tag: refs(tag).fwd),
                    POISONS[(k + int(p * 2)) % 2])
    mk.clear_plan_cache()


@pytest.mark.parametrize("name", ["sage", "gin"])
def test_capture_model_step(gpu, name):
    """A two-layer ``MaxKSAGE`` with ``feat_drop=0`` and a ``MaxKGIN`` in eval mode, forward and
    backward without an optimizer in one captured graph: output, input gradient and every
    parameter gradient after replay against the eager step, with the tolerance of the models'
    eager test (``test_layers.close`` at 2e-5; rocBLAS GEMMs and f32 accumulation orders differ
    from run to run, so nothing here is bit-equal)."""
    dst, src, n = small_edges(n=400, e=6000, seed=19)
    csr = mk.CSRGraph.from_edges(src.to(gpu), dst.to(gpu), n)
    torch.manual_seed(4)
    if name == "sage":
        model = MaxKSAGE(48, 64, 2, 7, 16, feat_drop=0.0, norm=True).to(gpu).train()
    else:
        model = MaxKGIN(48, 64, 2, 7, 16, feat_drop=0.5, norm=True).to(gpu).eval()
    params = dict(model.named_parameters())
    sets = {t: {"x": graphs.features(n, 48, seed=21 + j).numpy() * np.float32(4.0 ** j),
                "w": graphs.features(n, 7, seed=31 + j).numpy()} for j, t in enumerate(TAGS)}
    what = f"model {name}"

    def call(i, o):
        x = i["x"].requires_grad_(True)
        x.grad = None
        for q in params.values():
            q.grad = None
        y = model(csr, x)
        torch.autograd.backward([y], [i["w"]])
        return dict({"y": y.detach(), "gx": x.grad}, **{nm: q.grad for nm, q in params.items()})

    def check(tag, got, eager):
        if eager is None:
            assert all(np.isfinite(a).all() for a in got.values())
            return
        for nm, a in got.items():
            assert close(torch.from_numpy(a), torch.from_numpy(eager[nm]), 2e-5), \
                f"{what} {tag} {nm}"

    with torch.cuda.stream(side_stream()):          # the reference of the A / B precondition
        ref = {t: host(model(csr, to_dev(sets[t]["x"], gpu)).detach()) for t in "AB"}
    replay_protocol(case_of("autograd", what, sets=sets, outs=dict, call=call, check=check,
                            exact=False, main="y", ref=lambda tag: ref[tag]), POISONS[0])
    for q in params.values():
        q.grad = None
    mk.clear_plan_cache()


def test_values_are_a_snapshot(gpu):
    """The plan holds a snapshot of the edge values, and a replay reads the plan: after
    ``val.mul_(2)`` outside the capture a replay still computes with the values of capture time
    (the oracle on the old values). The host-side ``_version`` comparison of ``get_plan``, which
    a replay never runs, keeps working after a capture existed: an eager call made afterwards
    refreshes the plan and computes with the new values."""
    p, ix, v = exact_graph("empty")
    n, d, k = p.size - 1, 256, 16
    ptr, idx, val = graph_on(gpu, p, ix, v)
    r = forward_ref("empty", k, "range", "B")
    assert st.exactly_summable(2 * r.mag)
    sd, si = to_dev(r.od, gpu), to_dev(r.oi, gpu)
    s = side_stream()
    with torch.cuda.stream(s):
        ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d)        # builds the plan
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out, _ = ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d)
        val.mul_(2)
        out.fill_(float("nan"))
        g.replay()
        s.synchronize()
        assert_equal_floats(host(out), r.ref, "replay after val.mul_(2): the old values")
        eager, _ = ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d)
        s.synchronize()
        assert_equal_floats(host(eager), 2.0 * r.ref.astype(np.float64), "eager call: new values")
    del g
    mk.clear_plan_cache()
    COUNTS["forward"] += 1


# =========================================================================== refusals
def refused(fn, message):
    """``fn()`` inside a capture raises ``message`` before the refused call hands anything to the
    runtime. A torch kernel is recorded before it (with ``edge_weight=`` torch's own multiply of
    the values comes on top), so the graph is not empty; replaying it shows that the capture
    ended cleanly and nothing half-captured was left behind."""
    s = side_stream()
    marker = torch.zeros(1, device=DEV[0])
    with torch.cuda.stream(s):
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match=message):
            with torch.cuda.graph(g, stream=s):
                marker.add_(1)
                fn()
        assert not torch.cuda.is_current_stream_capturing()
        g.replay()
        s.synchronize()
        assert marker.item() == 1.0
    del g
    COUNTS["refusals"] += 1


def test_refuses_plan_build_during_capture(gpu):
    p, ix, v = exact_graph("empty")
    n, d, k = p.size - 1, 256, 16
    ptr, idx, val = graph_on(gpu, p, ix, v)
    r = forward_ref("empty", k, "range", "B")
    sd, si = to_dev(r.od, gpu), to_dev(r.oi, gpu)
    mk.clear_plan_cache()
    msg = r"build the plan before capture \(call once eagerly\)"
    refused(lambda: mk.GraphPlan(ptr, idx, val, n, ix.size, d, k), msg)
    refused(lambda: ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d), msg)  # cold cache
    assert ops.cached_plan_bytes() == 0
    with torch.cuda.stream(side_stream()):
        out, _ = ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d)
        side_stream().synchronize()
    assert_equal_floats(host(out), r.ref, "eager call after the refusal")
    mk.clear_plan_cache()


def test_refuses_value_refresh_during_capture(gpu):
    """``refresh_values`` itself, ``get_plan`` after an in-place edit of ``val``, and
    ``edge_weight=``."""
    p, ix, v = exact_graph("empty")
    n, d, k = p.size - 1, 256, 16
    ptr, idx, val = graph_on(gpu, p, ix, v)
    graph = mk.CSRGraph(ptr, idx, val)
    r = forward_ref("empty", k, "range", "B")
    sd, si = to_dev(r.od, gpu), to_dev(r.oi, gpu)
    ew = torch.full((ix.size,), 2.0, device=gpu)
    x = to_dev(r.x, gpu)
    msg = r"refresh_values .* cannot run while a graph is being captured: .* capture time"
    with torch.cuda.stream(side_stream()):
        plan = graph.plan(d, k)
        mk.spgemm(sd, si, graph, d, edge_weight=ew)                  # builds the weighted plan
        side_stream().synchronize()
    refused(lambda: plan.refresh_values(val), msg)
    refused(lambda: mk.spgemm(sd, si, graph, d, edge_weight=ew), msg)
    refused(lambda: mk.maxk_aggregate(x, graph, k, edge_weight=ew), msg)
    with torch.cuda.stream(side_stream()):
        val.mul_(2)
        side_stream().synchronize()
    refused(lambda: ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d), msg)
    with torch.cuda.stream(side_stream()):
        out, _ = ops.spgemm_forward(ptr, idx, val, sd, si, n, ix.size, k, d)
        y = mk.spgemm(sd, si, graph, d, edge_weight=ew)
        side_stream().synchronize()
    assert_equal_floats(host(out), 2.0 * r.ref.astype(np.float64), "eager call after the refusal")
    assert_equal_floats(host(y), 4.0 * r.ref.astype(np.float64), "edge_weight after the refusal")
    mk.clear_plan_cache()


def test_refuses_drawn_dropout_seed_during_capture(gpu):
    """``seed=None`` while training with ``dropout_p > 0``; an explicit seed, eval mode and
    ``dropout_p = 0`` stay accepted (test_capture_autograd_step captures them)."""
    gname, k = "empty", 32
    p, ix, v = exact_graph(gname)
    graph = mk.CSRGraph(*graph_on(gpu, p, ix, v))
    r = step_ref(gname, k, "exact", 0.5, False, "B")
    x = to_dev(r.x, gpu)
    with torch.cuda.stream(side_stream()):
        mk.maxk_aggregate(x, graph, k)                               # builds the plan
        side_stream().synchronize()
    msg = "pass seed=; a captured step replays one mask"
    refused(lambda: mk.maxk_aggregate(x, graph, k, dropout_p=0.5), msg)
    refused(lambda: mk.maxk_self_aggregate(x, graph, k, dropout_p=0.5), msg)
    refused(lambda: mk.maxk(x, k, dropout_p=0.5), msg)
    with torch.cuda.stream(side_stream()):
        y = mk.maxk_aggregate(x, graph, k, dropout_p=0.5, seed=SEED)
        mk.maxk_aggregate(x, graph, k, dropout_p=0.5)                # eager: a drawn seed is fine
        side_stream().synchronize()
    assert st.exactly_summable(r.fwd_mag)
    assert_equal_floats(host(y), r.fwd, "eager call after the refusal")
    mk.clear_plan_cache()


# =========================================================================== what ran
def test_capture_case_counts(gpu):
    """Runs last (file order): one line of case counts per family."""
    for family, count in COUNTS.items():
        print(f"capture: {family}: {count} cases")
    print(f"capture: {time.time() - T0:.0f} s since the module was imported")
