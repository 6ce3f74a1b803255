"""CPU: the max aggregation entry points are declared, bound and refuse bad arguments on the host
(null device pointers throughout: nothing reaches a GPU); the restatements of
tests/max_aggregate.py agree with each other; the exact-input cases of the GPU tests contain
every kind of output element the contract distinguishes; the maxk_mx:: fixture is the library's
set; and MaxKSAGEConv accepts the pool and gcn aggregators without changing a mean layer."""
import ctypes
import hashlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import max_aggregate as mx
import maxk_kernels as mk
from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_max.txt")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_max_aggregate_forward", "maxk_max_aggregate_backward", "maxk_max_row_limits")
P = ctypes.c_void_p
lib = _lib.lib
INVALID = -1
I32MAX = 2 ** 31 - 1


def err():
    return lib.maxk_last_error().decode()


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "Max aggregation (ABI 4)" in open(HEADER).read()
    assert lib.maxk_abi_version() == 4
    for name in ("max_aggregate", "maxk_max_aggregate", "dense_max_aggregate",
                 "MaxAggregateFunction", "max_row_limits"):
        assert name in mk.__all__ and hasattr(mk, name), name
    assert hasattr(torch.ops.maxk, "max_aggregate")
    assert hasattr(torch.ops.maxk, "max_aggregate_backward")


def test_row_limits():
    assert lib.maxk_max_row_limits(None, 0) == 4
    buf = (ctypes.c_int32 * 6)(*([-7] * 6))
    assert lib.maxk_max_row_limits(ctypes.cast(buf, P), 3) == 4
    assert list(buf) == list(mx.LIMITS[:3]) + [-7] * 3
    assert lib.maxk_max_row_limits(ctypes.cast(buf, P), 6) == 4
    assert tuple(buf[:4]) == mx.LIMITS and buf[4] == -7
    assert mk.max_row_limits() == mx.LIMITS


def fwd(ptr=None, idx=None, data=None, ds=0, sel=None, is_=0, out=None, ae=None, sl=None, n=10,
        nc=10, e=100, D=256, k=16):
    return lib.maxk_max_aggregate_forward(ptr, idx, data, ds, sel, is_, out, ae, sl, n, nc, e, D,
                                          k, None)


def bwd(pt=None, it=None, order=None, g=None, gs=0, ae=None, sl=None, sel=None, is_=0, gsp=None,
        n=10, nc=10, e=100, D=256, k=16):
    return lib.maxk_max_aggregate_backward(pt, it, order, g, gs, ae, sl, sel, is_, gsp, n, nc, e,
                                           D, k, None)


# the refusals of the multi-head aggregation that apply here (no heads, so none of theirs, and no
# multiple of 4 is asked of dim_origin)
BAD_SHAPES = [
    (dict(n=-1), "sizes"), (dict(nc=-1), "sizes"), (dict(e=-1), "sizes"),
    (dict(e=I32MAX + 1), "sizes"),
    (dict(nc=0), "without columns"), (dict(n=0), "without rows"),
    (dict(k=0), "k must be"), (dict(k=257), "k must be"), (dict(D=8, k=9), "k must be"),
    (dict(D=260, k=16), "dim_origin"), (dict(D=0), "dim_origin"),
    (dict(is_=15), "index_stride"),
    (dict(), "null pointer"),                                   # edges, and every pointer null
]


@pytest.mark.parametrize("call", [fwd, bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("kw,msg", BAD_SHAPES)
def test_refusals_on_the_host(call, kw, msg):
    extra = dict(gsp=P(4096)) if call is bwd and not kw else {}
    got = call(**kw, **extra)
    assert got == INVALID, (kw, got, err())
    assert msg in err(), err()


def test_strides_null_outputs_and_single_arg():
    assert fwd(ds=15) == INVALID and "data_stride" in err()
    assert bwd(gs=255, gsp=P(4096)) == INVALID and "grad_stride" in err()
    # arg_edge and arg_slot come together or not at all
    assert fwd(out=P(4096), ae=P(8192)) == INVALID and "both" in err()
    assert fwd(out=P(4096), sl=P(8192)) == INVALID and "both" in err()
    # a NULL out / grad_sp
    assert fwd(e=0) == INVALID and "null pointer" in err()
    assert bwd(e=0) == INVALID and "null pointer" in err()
    assert bwd() == INVALID and "null pointer" in err()
    # no rows / no columns with null pointers: nothing is dereferenced
    assert fwd(n=0, e=0) == 0 and bwd(nc=0, e=0) == 0
    # any dim_origin is served: an odd one gets as far as the pointer checks
    assert fwd(D=101, k=7) == INVALID and "null pointer" in err()


def test_overlapping_ranges_are_refused():
    base = 1 << 20
    a = dict(ptr=P(base), idx=P(base + 4096), data=P(base + 8192), sel=P(base + 12288),
             out=P(base + (1 << 16)), ae=P(base + (2 << 16)), sl=P(base + (3 << 16)))
    for name in ("ptr", "idx", "data", "sel"):
        for out in ("out", "ae", "sl"):
            bad = dict(a, **{out: P(a[name].value + 4)})
            assert fwd(**bad) == INVALID and "overlaps" in err(), (name, out)
    for x, y in (("ae", "out"), ("sl", "out"), ("sl", "ae")):
        bad = dict(a, **{x: P(a[y].value + 8)})
        assert fwd(**bad) == INVALID and "overlaps" in err(), (x, y)
    # without arg_*, out alone is checked
    assert fwd(**dict(a, ae=None, sl=None, out=P(a["idx"].value + 4))) == INVALID
    assert "overlaps" in err()
    # no edges: the outputs still may not overlap each other
    assert fwd(**dict(a, e=0, ae=P(a["out"].value + 8))) == INVALID and "overlaps" in err()
    b = dict(pt=P(base), it=P(base + 4096), order=P(base + 8192), g=P(base + (1 << 16)),
             ae=P(base + (2 << 16)), sl=P(base + (3 << 16)), sel=P(base + (4 << 16)),
             gsp=P(base + (5 << 16)))
    for name in ("pt", "it", "order", "g", "ae", "sl", "sel"):
        bad = dict(b, gsp=P(b[name].value + 4))
        assert bwd(**bad) == INVALID and "overlaps" in err(), name


# ------------------------------------------------------------------ restatements
def same(a, b):
    return all(np.array_equal(mx.bits(x) if x.dtype == np.float32 else x,
                              mx.bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


def test_order_key_is_the_order_of_the_contract():
    v = np.array([-np.inf, -4.0, -1e-45, -0.0, 0.0, 1e-45, 0.5, np.inf, np.nan], np.float32)
    key = mx.order_key(v).astype(np.int64)
    assert (np.diff(key) > 0).all() and key.min() > 0 and key[4] == int(mx.KEY_ZERO)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], np.uint32).view(np.float32)
    assert (mx.order_key(nans) == 0xffffffff).all()


def test_restatements_agree_with_each_other():
    ptr, idx = mx.small_graph(40)
    for D, k in ((64, 8), (100, 10), (256, 16), (8, 8), (256, 1)):
        for exact in (True, False):
            data, sel = mx.tables(40, D, k, seed=D + k, exact=exact)
            ref = mx.forward_ref(ptr, idx, data, sel, D)
            assert same(ref, mx.dense_ref(ptr, idx, data, sel, D)), (D, k, exact)
            out, ae, sl = ref
            # the winner's own bits, and nothing but zeros where the implicit zero won
            won = ae >= 0
            r, s = np.nonzero(won)
            assert np.array_equal(mx.bits(out[won]), mx.bits(data[idx[ae[won]], sl[won]]))
            assert np.array_equal(sel[idx[ae[won]], sl[won]], s)
            assert ((ae[won] >= ptr[r]) & (ae[won] < ptr[r + 1])).all()
            assert not mx.bits(out[~won]).any() and not sl[~won].any()
            # exactly one receiver: the backward hands on every element with a winner, once
            g = mx.exact_grad(40, D, seed=k)
            gsp, mag, m = mx.backward64(ptr, idx, g, ae, sl, sel)
            assert gsp.sum() == g[won].astype(np.float64).sum()
            assert m.sum() == np.count_nonzero(g[won])
    # a row without edges
    out, ae, sl = mx.forward_ref(np.zeros(3, np.int32), np.zeros(0, np.int32), data, sel, D)
    assert not mx.bits(out).any() and (ae == -1).all() and not sl.any()


@pytest.mark.parametrize("D,k", mx.SHAPES)
def test_exact_cases_contain_every_kind_of_element(D, k):
    """The precondition of the GPU tests: on the exact inputs of every shape an implicit zero
    wins, an explicit negative wins, an explicit 0.0 ties the implicit zero, and ties are
    resolved by edge position and within a multi-edge. With identity selectors every column
    selects every feature, so the implicit zero never competes in a row with edges: the two
    kinds that need it cannot occur there, which is asserted instead."""
    ptr, idx = mx.graph_arrays()
    data, sel, pre = mx.exact_analysis(D, k)
    out, ae, sl = mx.forward_ref(ptr, idx, data, sel, D, pre)
    got = mx.classes(ptr, idx, data, sel, D, out, ae, sl, pre)
    identity = (D, k) in mx.IDENTITY_SHAPES
    want = dict(implicit=not identity, negative=True, zero_tie=not identity, edge_tie=True,
                multi_edge_tie=True, slot_tie=False)
    assert got == want, got
    assert (np.diff(ptr) == 0).sum() >= 2 and (ae[np.diff(ptr) == 0] == -1).all()


def test_repeated_selector_tables_tie_by_slot():
    ptr, idx = mx.graph_arrays()
    for make, D, k in ((mx.repeated_tables, 256, 16), (mx.repeated_tables, 256, 100),
                       (mx.padded_tables, 64, 8)):
        data, sel = make(D, k, seed=5)
        assert (np.diff(np.sort(sel, axis=1), axis=1) == 0).any(axis=1).sum() >= mx.NUM // 6
        got = mx.classes(ptr, idx, data, sel, D, *mx.forward_ref(ptr, idx, data, sel, D))
        assert got["slot_tie"] and got["implicit"] and got["edge_tie"], (make.__name__, got)


# ------------------------------------------------------------------ selectors, fixtures
def test_restated_selectors_cover_the_fixture():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_mx::") for n in names)
    fwd_names = {mx.fwd_kernel_name(k, arg) for k in range(1, 257) for arg in (False, True)}
    bwd_names = {mx.bwd_kernel_name(k) for k in range(1, 257)}
    assert fwd_names | bwd_names == set(names)
    assert len(fwd_names) == 8 and len(bwd_names) == 4
    # the GPU module's shapes reach every one of them (each runs with and without arg_*)
    assert {mx.fwd_kernel_name(k, arg) for _, k in mx.SHAPES for arg in (False, True)} == fwd_names
    assert {mx.bwd_kernel_name(k) for _, k in mx.SHAPES} == bwd_names


def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_mx::") == kernel_list.read_list(FIXTURE)


def test_wrapper_checks_the_longest_row_once():
    """Rows of 2^24 edges or more are refused by max_aggregate before any launch; the answer is
    cached on the CSRGraph, and a graph with fewer edges than that is not looked at."""
    from maxk_kernels import ops, pooling
    e = ops.MAX_ROW_EDGES
    idx = torch.zeros(e, dtype=torch.int32)
    long = mk.CSRGraph(torch.tensor([0, e, e], dtype=torch.int32), idx)
    with pytest.raises(RuntimeError, match="rows must be shorter"):
        pooling._check_rows(long)
    assert long._values["max_row_edges"] == e
    data, sel = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="rows must be shorter"):
        mk.max_aggregate(long, data, sel, 8)
    halves = mk.CSRGraph(torch.tensor([0, e // 2, e], dtype=torch.int32), idx)
    pooling._check_rows(halves)
    assert halves._values["max_row_edges"] == e // 2
    small = mk.CSRGraph(torch.tensor([0, 3, 3], dtype=torch.int32), idx[:3])
    pooling._check_rows(small)
    assert "max_row_edges" not in small._values


# ------------------------------------------------------------------ layer constructor
def digest(state):
    h = hashlib.sha256()
    for key, v in state.items():
        h.update(key.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def test_layer_constructor():
    # a mean / sum layer is what it was before the new aggregators: keys, seeded weights and the
    # position of the random stream afterwards (literals taken at the parent commit)
    for agg in ("mean", "sum"):
        torch.manual_seed(1234)
        layer = mk.MaxKSAGEConv(48, 64, agg)
        assert list(layer.state_dict()) == ["bias", "fc_self.weight", "fc_neigh.weight"]
        assert digest(layer.state_dict()) == "113fb43ca3792da5"
        assert float(torch.rand(1)) == 0.4580006003379822
    pool = mk.MaxKSAGEConv(48, 64, "pool")
    assert list(pool.state_dict()) == ["bias", "fc_self.weight", "fc_neigh.weight",
                                       "fc_pool.weight", "fc_pool.bias"]
    assert pool.fc_pool.weight.shape == (48, 48) and pool.fc_pool.bias.shape == (48,)
    gcn = mk.MaxKSAGEConv(48, 64, "gcn")
    assert list(gcn.state_dict()) == ["bias", "fc_neigh.weight"] and not hasattr(gcn, "fc_self")
    assert not hasattr(mk.MaxKSAGEConv(48, 64, "mean"), "fc_pool")
    for bad in ("lstm", "max", ""):
        with pytest.raises(ValueError, match="Unsupported aggregator type"):
            mk.MaxKSAGEConv(48, 64, bad)
    for agg in ("pool", "gcn"):
        with pytest.raises(ValueError, match="maxk_after_fc"):
            mk.MaxKSAGEConv(48, 64, agg, maxk_after_fc=True)
        mk.MaxKSAGEConv(48, 64, agg, nonlinear="relu")
    model = mk.MaxKSAGE(32, 48, 2, 7, maxk=8, aggregator_type="pool")
    assert all(layer.aggregator_type == "pool" for layer in model.layers)
    assert all(layer.aggregator_type == "mean" for layer in mk.MaxKSAGE(32, 48, 2, 7).layers)
