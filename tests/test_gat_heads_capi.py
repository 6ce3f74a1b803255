"""CPU: the head-batched attention and multi-head aggregation entry points are declared, bound
and refuse bad arguments on the host (null device pointers throughout: nothing reaches a GPU);
the float64 restatements of tests/gat_heads.py agree with a dense composition; a sequential f32
summation stays inside each derived bound (the precondition of the GPU bound tests); the exact
inputs are exactly summable; and the maxk_mh:: fixture is the library's set."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import gat_heads as gh
from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_heads.txt")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_gat_attention_forward_heads", "maxk_gat_attention_backward_heads",
       "maxk_edge_colsum_heads", "maxk_heads_aggregate_forward", "maxk_heads_aggregate_backward",
       "maxk_heads_row_limits")
P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
I32MAX = 2 ** 31 - 1


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "GAT attention, heads" in open(HEADER).read()
    assert "Multi-head aggregation" in open(HEADER).read()


def test_row_limits():
    assert lib.maxk_heads_row_limits(None, 0) == 4
    buf = (ctypes.c_int32 * 6)(*([-7] * 6))
    assert lib.maxk_heads_row_limits(ctypes.cast(buf, P), 3) == 4
    assert list(buf) == list(gh.LIMITS[:3]) + [-7] * 3
    assert lib.maxk_heads_row_limits(ctypes.cast(buf, P), 6) == 4
    assert tuple(buf[:4]) == gh.LIMITS and buf[4] == -7


def fwd(ptr=None, idx=None, alpha=None, data=None, ds=0, sel=None, is_=0, out=None, H=8, n=10,
        nc=10, e=100, D=256, k=16):
    return lib.maxk_heads_aggregate_forward(ptr, idx, alpha, data, ds, sel, is_, out, H, n, nc, e,
                                            D, k, None)


def bwd(pt=None, it=None, order=None, alpha=None, g=None, gs=0, data=None, ds=0, sel=None, is_=0,
        gsp=None, ga=None, H=8, n=10, nc=10, e=100, D=256, k=16):
    return lib.maxk_heads_aggregate_backward(pt, it, order, alpha, g, gs, data, ds, sel, is_, gsp,
                                             ga, H, n, nc, e, D, k, None)


BAD_SHAPES = [
    (dict(n=-1), INVALID, "sizes"), (dict(nc=-1), INVALID, "sizes"), (dict(e=-1), INVALID, "sizes"),
    (dict(e=I32MAX + 1), INVALID, "sizes"),
    (dict(nc=0), INVALID, "without columns"),
    (dict(k=0), INVALID, "k must be"), (dict(k=257), INVALID, "k must be"),
    (dict(D=260, k=16, H=5), INVALID, "dim_origin"), (dict(D=0), INVALID, "dim_origin"),
    (dict(H=0), INVALID, "num_heads"), (dict(H=-3), INVALID, "num_heads"),
    (dict(H=3), INVALID, "num_heads"),                         # 3 does not divide 256
    (dict(ds=15), INVALID, "data_stride"), (dict(is_=15), INVALID, "index_stride"),
    (dict(D=96, H=16, k=8), UNSUPPORTED, "multiple of 4"),      # F = 6
    (dict(D=256, H=32, k=8), UNSUPPORTED, "above 16"),
    (dict(), INVALID, "null pointer"),                          # edges, and every pointer null
]


@pytest.mark.parametrize("call", [fwd, bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("kw,rc,msg", BAD_SHAPES)
def test_aggregate_refusals_on_the_host(call, kw, rc, msg):
    extra = dict(gsp=P(4096)) if call is bwd and not kw else {}
    got = call(**kw, **extra)
    assert got == rc, (kw, got, lib.maxk_last_error().decode())
    assert msg in lib.maxk_last_error().decode(), lib.maxk_last_error().decode()


def test_backward_stride_and_null_outputs():
    assert bwd(gs=255, gsp=P(4096)) == INVALID and "grad_stride" in lib.maxk_last_error().decode()
    # both outputs NULL: nothing to do, whatever else is null
    assert bwd() == 0
    # no rows / no columns / no edges with null pointers: nothing is dereferenced
    assert fwd(n=0, e=0) == 0 and bwd(nc=0, e=0, gsp=P(4096)) == 0
    assert fwd(e=0) == INVALID and "null pointer" in lib.maxk_last_error().decode()  # out is NULL


def test_overlapping_ranges_are_refused():
    n = nc = 10
    e, D, k, H = 100, 256, 16, 8
    base = 1 << 20
    a = dict(ptr=P(base), idx=P(base + 4096), alpha=P(base + 8192), data=P(base + 16384),
             sel=P(base + 20480), out=P(base + 32768))
    for name in ("ptr", "idx", "alpha", "data", "sel"):
        bad = dict(a, out=P(a[name].value + 4))
        assert fwd(**bad) == INVALID and "overlaps" in lib.maxk_last_error().decode(), name
    b = dict(pt=P(base), it=P(base + 4096), order=P(base + 8192), alpha=P(base + 12288),
             g=P(base + 20480), data=P(base + 36864), sel=P(base + 40960),
             gsp=P(base + 45056), ga=P(base + 49152))
    for name in ("pt", "it", "order", "alpha", "g", "data", "sel"):
        for out in ("gsp", "ga"):
            bad = dict(b, **{out: P(b[name].value + 4)})
            assert bwd(**bad) == INVALID and "overlaps" in lib.maxk_last_error().decode(), \
                (name, out)
    bad = dict(b, ga=P(b["gsp"].value + 8))
    assert bwd(**bad) == INVALID and "overlaps" in lib.maxk_last_error().decode()
    # alpha is not read without grad_sp, sp_data not without grad_alpha: no overlap to refuse,
    # and a null one is no error (the call would then launch, so it is not made here)
    assert n * nc * e * D * k * H > 0


def test_batched_attention_refusals_on_the_host():
    f = lib.maxk_gat_attention_forward_heads
    b = lib.maxk_gat_attention_backward_heads
    c = lib.maxk_edge_colsum_heads
    for H, msg in ((0, "num_heads must be >= 1"), (-2, "num_heads must be >= 1"),
                   (65536, "beyond"), (I32MAX, "beyond")):
        assert f(None, None, None, None, 0.2, None, H, 10, 10, I32MAX, None) == INVALID
        assert msg in lib.maxk_last_error().decode()
        assert b(None, None, None, None, 0.2, None, None, None, None, H, 10, 10, I32MAX,
                 None) == INVALID
        assert msg in lib.maxk_last_error().decode()
        assert c(None, None, None, None, H, 10, I32MAX, None) == INVALID
        assert msg in lib.maxk_last_error().decode()
    # the single-head refusals, unchanged in the batched calls
    assert f(None, None, None, None, 0.2, None, 4, 10, 10, 100, None) == INVALID
    assert "null pointer" in lib.maxk_last_error().decode()
    assert f(None, None, None, None, float("nan"), None, 4, 10, 10, 100, None) == INVALID
    assert f(None, None, None, None, 0.2, None, 4, 10, 0, 100, None) == INVALID
    assert f(None, None, None, None, 0.2, None, 4, -1, 10, 100, None) == INVALID
    assert f(None, None, None, None, 0.2, None, 4, 10, 10, I32MAX + 1, None) == INVALID
    assert c(None, None, None, None, 4, 10, 100, None) == INVALID
    assert f(None, None, None, None, 0.2, None, 4, 10, 10, 0, None) == 0
    # head-major extents enter the overlap check: alpha of 4 heads reaches into el
    base, e = 1 << 20, 100
    assert f(P(base), P(base + 4096), P(base + 8192 + 4 * e * 3), P(base + 65536), 0.2,
             P(base + 8192), 4, 10, 10, e, None) == INVALID
    assert "overlaps" in lib.maxk_last_error().decode()


# ------------------------------------------------------------------ restatements and bounds
def test_restatement_agrees_with_the_dense_composition():
    ptr, idx = gh.small_graph(40)
    for D, H, k in ((64, 2, 8), (96, 3, 10), (256, 8, 16)):
        data, sel = gh.tables(40, D, k, seed=k, exact=False)
        alpha = np.random.default_rng(H).random((H, idx.size)).astype(np.float32)
        out, mag, m = gh.forward64(ptr, idx, alpha, data, sel, D)
        dense = gh.dense_forward64(ptr, idx, alpha, data, sel, D)
        assert np.allclose(out, dense, rtol=1e-12, atol=1e-12 * mag.max())
        assert (m <= np.diff(ptr)[:, None]).all() and (mag >= np.abs(out) - 1e-12).all()
        # the gradients are the adjoints: <g, out> = <grad_sp, data> = <grad_alpha, alpha>
        g = np.random.default_rng(k).standard_normal((40, D)).astype(np.float32)
        (gsp, _, sm), (ga, _, am) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
        lhs = float((g.astype(np.float64) * out).sum())
        assert np.isclose(lhs, float((gsp * data).sum()), rtol=1e-10)
        assert np.isclose(lhs, float((ga * alpha).sum()), rtol=1e-10)
        assert am.max() <= k and (sm <= np.bincount(idx, minlength=40)[:, None]).all()


def test_magic_head_of_feature_is_exact():
    """(s * (65536 // F + 1)) >> 16 == s // F for every feature and every supported F
    (csrc/variants_heads.h, heads_head_of)."""
    s = np.arange(256, dtype=np.int64)
    for F in range(4, 257, 4):
        assert np.array_equal((s * (65536 // F + 1)) >> 16, s // F), F


@pytest.mark.parametrize("n", [1, 2, 17, 513, 5000, 45000])
def test_sequential_f32_summation_is_within_the_bound(n):
    """The derived bound (m + 4) u sum |terms| against a sequential f32 summation of f32-rounded
    products: the worst order a kernel could take short of a tree."""
    rng = np.random.default_rng(n)
    worst = 0.0
    for _ in range(8):
        a = rng.random(n).astype(np.float32)
        x = rng.standard_normal(n).astype(np.float32)
        exact = float((a.astype(np.float64) * x).sum())
        got = float(gh.sequential_f32(a * x))
        bnd = float(gh.bound(np.abs(a.astype(np.float64) * x).sum(), float(n)))
        worst = max(worst, abs(got - exact) / bnd)
    print(f"\nsequential f32, n = {n}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_exact_inputs_are_exactly_summable():
    ptr, idx = gh.graph_arrays()
    D, H, k = 256, 8, 16
    data, sel = gh.tables(gh.NUM, D, k, seed=1, exact=True)
    alpha = gh.exact_alpha(H, idx.size, 2)
    g = gh.exact_grad(gh.NUM, D, 3)
    out, mag, _ = gh.forward64(ptr, idx, alpha, data, sel, D)
    (gsp, smag, _), (ga, amag, _) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    for v, mg in ((out, mag), (gsp, smag), (ga, amag)):
        assert mg.max() * 8 < 2 ** 23                     # quanta of 1/8
        assert np.array_equal(v * 8, np.round(v * 8)) and np.array_equal(v.astype(np.float32), v)
    rlen, clen = np.diff(ptr), np.bincount(idx, minlength=gh.NUM)
    for lens in (rlen, clen):
        for want in (0, 1, 2) + tuple(l + d for l in gh.LIMITS[:2] for d in (-1, 0, 1)):
            assert (lens == want).any(), want
    assert rlen.max() == gh.HUB_ROW and clen.max() == gh.HUB_COL


# ------------------------------------------------------------------ selectors, fixtures
def test_restated_selectors_cover_the_fixture():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_mh::") for n in names)
    fwd_names = {gh.fwd_kernel_name(k) for k in range(1, 257)}
    bwd_names = {gh.bwd_kernel_name(k, H) for k in range(1, 257) for H in range(1, 17)}
    assert fwd_names | bwd_names | set(gh.ATTENTION_KERNELS) == set(names)
    assert len(fwd_names) == 4 and len(bwd_names) == 7
    # the GPU module's shapes reach every one of them
    assert {gh.fwd_kernel_name(k) for _, _, k in gh.SHAPES} == fwd_names
    assert {gh.bwd_kernel_name(k, H) for _, H, k in gh.SHAPES} == bwd_names


def test_fixtures_equal_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_mh::") == kernel_list.read_list(FIXTURE)
    main = os.path.join(ROOT, "tests", "golden", "kernel_instantiations.txt")
    assert kernel_list.compiled(_lib.LIB_PATH) == kernel_list.read_list(main)
    assert kernel_list.ours(["void maxk_mh::f<8>(int)", "void maxk::g(int)"],
                            prefix="maxk_mh::") == ["maxk_mh::f<8>"]
    assert kernel_list.ours(["void maxk_mh::f<8>(int)", "void maxk::g(int)"]) == ["maxk::g"]
