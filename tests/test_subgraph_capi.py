"""CPU: the induced-subgraph entry points are declared, bound and refuse bad arguments on the host
(null or made-up device pointers: nothing reaches a GPU); the numpy restatement of
tests/subgraph.py holds the properties the rule promises; the node sets hold the preconditions of
the GPU cases; random_partition, ClusterLoader and Subgraph behave on the host as documented (the
loader with the restatement in the kernel's place: node_subgraph itself needs a device); and the
maxk_sg:: fixture is the library's set."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import maxk_kernels as mk
import subgraph as sg
from maxk_kernels import _lib, ops
from maxk_kernels import subgraph as mksub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_subgraph.txt")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_induced_subgraph_scratch_bytes", "maxk_induced_subgraph_count",
       "maxk_induced_subgraph_fill", "maxk_subgraph_row_limits")
P = ctypes.c_void_p
lib = _lib.lib
INVALID = -1
I32MAX = 2 ** 31 - 1
BASE = 1 << 20


def err():
    return lib.maxk_last_error().decode()


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "Induced subgraphs (ABI 4)" in open(HEADER).read()
    assert lib.maxk_abi_version() == 4
    for name in ("node_subgraph", "Subgraph", "random_partition", "ClusterLoader",
                 "subgraph_row_limits"):
        assert name in mk.__all__ and hasattr(mk, name), name
    assert callable(ops.induced_subgraph_count) and callable(ops.induced_subgraph_fill)
    assert callable(ops.subgraph_row_limits)


def test_row_limits_and_scratch_sizes():
    assert lib.maxk_subgraph_row_limits(None, 0) == 2
    buf = (ctypes.c_int32 * 4)(*([-7] * 4))
    assert lib.maxk_subgraph_row_limits(ctypes.cast(buf, P), 1) == 2
    assert list(buf) == [sg.LIMITS[0], -7, -7, -7]
    assert lib.maxk_subgraph_row_limits(ctypes.cast(buf, P), 4) == 2
    assert tuple(buf[:2]) == sg.LIMITS and buf[2] == -7
    assert mk.subgraph_row_limits() == sg.LIMITS == ops.subgraph_row_limits()
    for n in (0, 1, 600, 232965, 2449029):
        for s in (0, 1, 2046, 2047, 2048, 65536, 10 ** 6):
            assert lib.maxk_induced_subgraph_scratch_bytes(n, s) == sg.scratch_bytes(n, s), (n, s)
            assert ops.induced_subgraph_scratch_bytes(n, s) == sg.scratch_bytes(n, s)
    assert lib.maxk_induced_subgraph_scratch_bytes(-1, 5) == 0
    assert lib.maxk_induced_subgraph_scratch_bytes(5, -1) == 0


# ------------------------------------------------------------------ refusals
def count(ptr=P(BASE), idx=P(BASE + (1 << 16)), nodes=P(BASE + (2 << 16)),
          out_ptr=P(BASE + (3 << 16)), counts=P(BASE + (4 << 16)), scratch=P(BASE + (5 << 16)),
          sb=None, n=600, e=5000, s=100):
    sb = sg.scratch_bytes(max(n, 0), max(s, 0)) if sb is None else sb
    return lib.maxk_induced_subgraph_count(ptr, idx, nodes, out_ptr, counts, scratch, sb, n, e, s,
                                           None)


def fill(ptr=P(BASE), idx=P(BASE + (1 << 16)), nodes=P(BASE + (2 << 16)),
         out_ptr=P(BASE + (3 << 16)), col=P(BASE + (4 << 16)), eid=P(BASE + (5 << 16)), cap=1000,
         scratch=P(BASE + (6 << 16)), sb=None, n=600, e=5000, s=100):
    sb = sg.scratch_bytes(max(n, 0), max(s, 0)) if sb is None else sb
    return lib.maxk_induced_subgraph_fill(ptr, idx, nodes, out_ptr, col, eid, cap, scratch, sb, n,
                                          e, s, None)


COMMON_REFUSALS = [
    (dict(s=-1), "negative number of selected nodes"),
    (dict(n=-1), "sizes"), (dict(e=-1), "sizes"), (dict(e=I32MAX + 1), "sizes"),
    (dict(n=0), "empty graph"),
    (dict(sb=2000), "scratch_bytes"),
    (dict(ptr=None), "null pointer"), (dict(idx=None), "null pointer"),
    (dict(nodes=None), "null pointer"), (dict(out_ptr=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
]
COUNT_REFUSALS = COMMON_REFUSALS + [
    (dict(counts=None), "null pointer"),
    (dict(out_ptr=P(BASE + 4)), "overlaps"), (dict(out_ptr=P(BASE + (1 << 16) + 4)), "overlaps"),
    (dict(counts=P(BASE + (2 << 16) + 4)), "overlaps"),
    (dict(counts=P(BASE + (3 << 16) + 8)), "overlaps"),
    (dict(scratch=P(BASE + (3 << 16) + 4)), "overlaps"),
    (dict(scratch=P(BASE + (4 << 16) - 2000)), "overlaps"),
]
FILL_REFUSALS = COMMON_REFUSALS + [
    (dict(cap=I32MAX + 1), "fit int32"), (dict(cap=-1), "fit int32"),
    (dict(col=None), "null pointer"), (dict(eid=None), "null pointer"),
    (dict(col=P(BASE + 4)), "overlaps"), (dict(eid=P(BASE + (1 << 16) + 4)), "overlaps"),
    (dict(col=P(BASE + (2 << 16) + 4)), "overlaps"),
    (dict(eid=P(BASE + (3 << 16) + 4)), "overlaps"),          # out_ptr is an input of _fill
    (dict(eid=P(BASE + (4 << 16) + 8)), "overlaps"),
    (dict(scratch=P(BASE + (5 << 16) + 4)), "overlaps"),
]


@pytest.mark.parametrize("kw,msg", COUNT_REFUSALS)
def test_count_refusals_on_the_host(kw, msg):
    got = count(**kw)
    assert got == INVALID, (kw, got, err())
    assert msg in err() and "maxk_induced_subgraph_count" in err(), err()


@pytest.mark.parametrize("kw,msg", FILL_REFUSALS)
def test_fill_refusals_on_the_host(kw, msg):
    got = fill(**kw)
    assert got == INVALID, (kw, got, err())
    assert msg in err() and "maxk_induced_subgraph_fill" in err(), err()


def test_ops_check_their_tensors_before_the_library():
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.induced_subgraph_count(t, t, t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.induced_subgraph_fill(t, t, t, t, capacity=0)


# ------------------------------------------------------------------ the restatement
def test_header_states_the_rule():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    for phrase in ("local(c) is the lowest position i with nodes[i] == c",
                   "keeps exactly the edges e in [ptr[r], ptr[r + 1]) with local(idx[e]) != NONE, "
                   "in ascending e",
                   "the exclusive scan of the kept counts",
                   "its row is emitted once per position",
                   "clamped into [0, num_nodes) before any use"):
        assert phrase in text, phrase


def test_identity_set_gives_the_graph_back():
    ptr, idx, n = sg.graph()
    out_ptr, col, eid, counts = sg.reference("all")
    assert np.array_equal(out_ptr, ptr) and np.array_equal(col, idx)
    assert np.array_equal(eid, np.arange(idx.size, dtype=np.int32))
    assert counts == (idx.size, n, 0)


def test_a_permuted_set_is_the_symmetric_permutation_of_the_dense_matrix():
    ptr, idx, n = sg.graph()
    dense = sg.dense_of(ptr, idx, n)
    for name in ("permuted", "half", "few_columns", "every_column", "hub", "designed"):
        nodes = sg.node_sets()[name].astype(np.int64)
        out_ptr, col, eid, counts = sg.reference(name)
        assert np.array_equal(sg.dense_of(out_ptr, col, nodes.size), dense[nodes][:, nodes]), name
        assert np.array_equal(idx[eid], nodes[col]) and counts[1:] == (nodes.size, 0)
        for i in (0, nodes.size // 2, nodes.size - 1):      # edge order is the parent's
            mine = eid[out_ptr[i]:out_ptr[i + 1]].astype(np.int64)
            r = nodes[i]
            assert (np.diff(mine) > 0).all() and ((mine >= ptr[r]) & (mine < ptr[r + 1])).all()


def test_multigraph_rows_repeated_and_stray_nodes():
    # row 0 names column 2 three times and column 1 twice; row 2 has a self loop
    ptr = np.array([0, 6, 6, 9, 10], np.int32)
    idx = np.array([2, 1, 2, 3, 1, 2, 0, 2, 0, 3], np.int32)
    dense = sg.dense_of(ptr, idx, 4)
    for nodes in ([0, 2], [2, 0], [3, 1, 0], [0, 1, 2, 3], [1]):
        out_ptr, col, eid, counts = sg.subgraph_ref(ptr, idx, nodes, 4)
        assert np.array_equal(sg.dense_of(out_ptr, col, len(nodes)), dense[nodes][:, nodes])
        assert counts == (col.size, len(nodes), 0)
    out_ptr, col, eid, _ = sg.subgraph_ref(ptr, idx, [2, 0], 4)
    assert out_ptr.tolist() == [0, 3, 6] and col.tolist() == [1, 0, 1, 0, 0, 0]
    assert eid.tolist() == [6, 7, 8, 0, 2, 5]
    # a repeated node: its row once per position, its column numbered by the lowest position
    out_ptr, col, eid, counts = sg.subgraph_ref(ptr, idx, [2, 0, 2], 4)
    assert out_ptr.tolist() == [0, 3, 6, 9] and counts == (9, 2, 0)
    assert col.tolist() == [1, 0, 1, 0, 0, 0, 1, 0, 1] and eid.tolist() == [6, 7, 8, 0, 2, 5, 6, 7, 8]
    # entries out of range are clamped and counted
    got = sg.subgraph_ref(ptr, idx, [-5, 9, 2], 4)
    want = sg.subgraph_ref(ptr, idx, [0, 3, 2], 4)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    assert got[3] == (want[3][0], 3, 2)
    assert sg.subgraph_ref(ptr, idx, [], 4)[0].tolist() == [0]


def test_the_loop_free_count_equals_the_restatement():
    ptr, idx, n = sg.graph()
    for name in sorted(sg.node_sets()):
        want = sg.reference(name)
        got = sg.count_ref(ptr, idx, sg.node_sets()[name], n)
        assert np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and got[1] == want[3]
    for nodes in ([30, 40, 30, sg.HUB, 50, 40, 580], [30, n, -3, sg.HUB, 50, 2 ** 31 - 1, -2 ** 31]):
        want = sg.subgraph_ref(ptr, idx, nodes, n)
        got = sg.count_ref(ptr, idx, nodes, n)
        assert np.array_equal(got[0], want[0]) and got[1] == want[3], nodes


def test_node_sets_hold_the_preconditions_of_the_gpu_cases():
    """Selected rows of length 0, 1 and limit - 1 / at / + 1 of every limit the library reports,
    a hub; nothing, some and all of a row kept in each of the three regimes."""
    assert mk.subgraph_row_limits() == sg.LIMITS
    ptr, idx, n = sg.graph()
    sets = sg.node_sets()
    assert set(sets) == {"none", "isolated", "hub", "all", "permuted", "half", "designed",
                         "few_columns", "every_column"}
    seen, lengths = sg.kept_fractions()
    need = {0, 1, 5000}
    for limit in sg.LIMITS:
        need |= {limit - 1, limit, limit + 1}
    assert need <= lengths, sorted(need - lengths)
    assert seen == {(r, kind) for r in (0, 1, 2) for kind in ("nothing", "some", "all")}, seen
    lens = np.diff(ptr)
    for name in ("designed", "few_columns", "every_column"):
        assert set(sg.DESIGNED_ROWS) <= set(sets[name].tolist()), name
    assert need <= set(lens[list(sg.DESIGNED_ROWS)].tolist())
    assert sets["none"].size == 0 and sg.reference("none")[3] == (0, 0, 0)
    iso = int(sets["isolated"][0])
    assert lens[iso] == 0 and not (idx == iso).any()
    assert lens[sg.HUB] == 5000 and sg.reference("hub")[3] == (0, 1, 0)
    assert sg.reference("designed")[3][0] == 0
    for r in sg.DESIGNED_ROWS:                               # every edge of theirs kept
        i = sets["every_column"].tolist().index(r)
        out_ptr = sg.reference("every_column")[0]
        assert out_ptr[i + 1] - out_ptr[i] == lens[r]
    assert sorted(sets["permuted"].tolist()) == list(range(n))
    assert not np.array_equal(sets["permuted"], sets["all"])
    assert (np.diff(sets["half"]) > 0).all() and sets["half"].size == n // 2
    for nodes in sets.values():
        assert np.unique(nodes).size == nodes.size
    # rows start at every offset from a 16-byte boundary (the quads of the wide loads)
    assert {int(ptr[r]) % 4 for r in range(n) if lens[r] > 16} == {0, 1, 2, 3}


# ------------------------------------------------------------------ partition, loader, Subgraph
def test_random_partition_sizes_and_determinism():
    for n, p, seed in ((600, 4, 0), (601, 7, 3), (10, 10, 1), (5, 1, 9), (1000, 64, 2)):
        parts = mk.random_partition(n, p, seed)
        assert parts.dtype == torch.int32 and parts.shape == (n,) and parts.device.type == "cpu"
        sizes = torch.bincount(parts.long(), minlength=p)
        assert sizes.numel() == p and int(sizes.max()) - int(sizes.min()) <= 1
        assert int(sizes.sum()) == n and int(sizes.min()) >= 1
        assert torch.equal(parts, mk.random_partition(n, p, seed))
        # the stated rule
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
        want = torch.empty(n, dtype=torch.int64)
        want[perm] = torch.arange(n) * p // n
        assert torch.equal(parts.long(), want)
    assert not torch.equal(mk.random_partition(600, 4, 0), mk.random_partition(600, 4, 1))
    for bad in (0, -1, 11):
        with pytest.raises(ValueError, match="num_parts"):
            mk.random_partition(10, bad)


def cpu_graph():
    ptr, idx, _ = sg.graph()
    val = torch.arange(idx.size, dtype=torch.float32) + 1
    return mk.CSRGraph(torch.from_numpy(ptr.copy()), torch.from_numpy(idx.copy()), val)


def node_subgraph_on_the_host(graph, nodes):
    """node_subgraph with the restatement in the kernels' place (CPU tensors)."""
    nodes = nodes.to(torch.int32)
    out_ptr, col, eid, (m, distinct, stray) = sg.subgraph_ref(
        graph.ptr.numpy(), graph.idx.numpy(), nodes.numpy(), graph.num_nodes)
    assert stray == 0 and distinct == nodes.numel()
    eid = torch.from_numpy(eid)
    return mk.Subgraph(torch.from_numpy(out_ptr), torch.from_numpy(col), graph.val[eid.long()],
                       node_ids=nodes, eids=eid, parent_num_nodes=graph.num_nodes)


@pytest.fixture
def host_loader(monkeypatch):
    calls = []

    def fake(graph, nodes):
        calls.append(nodes.clone())
        return node_subgraph_on_the_host(graph, nodes)

    monkeypatch.setattr(mksub, "node_subgraph", fake)
    return calls


def test_cluster_loader_argument_errors():
    g = cpu_graph()
    n = g.num_nodes
    ok = mk.random_partition(n, 4, 0)
    with pytest.raises(ValueError, match="clusters_per_batch"):
        mk.ClusterLoader(g, ok, clusters_per_batch=0)
    holes = ok.clone()
    holes[holes == 2] = 5
    with pytest.raises(ValueError, match="empty parts"):
        mk.ClusterLoader(g, holes)
    neg = ok.clone()
    neg[3] = -1
    with pytest.raises(ValueError, match=r"\[0, P\)"):
        mk.ClusterLoader(g, neg)
    with pytest.raises(ValueError, match="one integer part id per node"):
        mk.ClusterLoader(g, ok[:-1])
    with pytest.raises(ValueError, match="one integer part id per node"):
        mk.ClusterLoader(g, ok.float())
    with pytest.raises(ValueError, match="num_parts"):
        mk.ClusterLoader(g, n + 1)
    with pytest.raises(TypeError, match="CSRGraph"):
        mk.ClusterLoader(object(), ok)
    block = mk.Block(torch.tensor([0, 1]), torch.tensor([2]), num_src=3)
    with pytest.raises(TypeError, match="CSRGraph"):
        mk.ClusterLoader(block, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="rectangular"):
        mk.node_subgraph(block, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="CSRGraph"):
        mk.node_subgraph(object(), torch.zeros(1, dtype=torch.int32))
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(TypeError, match="integer node ids"):
            mk.node_subgraph(g, bad)


def test_cluster_loader_batches_len_and_cache(host_loader):
    g = cpu_graph()
    n = g.num_nodes
    ptr, idx, _ = sg.graph()
    parts = mk.random_partition(n, 7, 5)
    for cpb in (1, 2, 3, 7, 9):
        loader = mk.ClusterLoader(g, parts, clusters_per_batch=cpb)
        assert len(loader) == -(-7 // cpb) and loader.num_parts == 7 and loader.cache
        first = list(loader)
        assert len(first) == len(loader) and loader.epoch == 1
        seen = []
        for b, sub in enumerate(first):
            clusters = list(range(b * cpb, min((b + 1) * cpb, 7)))
            want = torch.nonzero(torch.isin(parts, torch.tensor(clusters))).flatten()
            assert torch.equal(sub.node_ids.long(), want)            # ascending, the union
            ref = sg.subgraph_ref(ptr, idx, want.numpy(), n)
            assert np.array_equal(sub.ptr.numpy(), ref[0]) and np.array_equal(sub.idx.numpy(), ref[1])
            assert np.array_equal(sub.eids.numpy(), ref[2])
            seen.append(want)
        assert torch.equal(torch.sort(torch.cat(seen)).values, torch.arange(n))
        built = len(host_loader)
        second = list(loader)
        assert all(a is b for a, b in zip(first, second)) and len(host_loader) == built
    # one batch of all clusters is the graph itself
    whole = next(iter(mk.ClusterLoader(g, parts, clusters_per_batch=7)))
    assert torch.equal(whole.ptr, g.ptr) and torch.equal(whole.idx, g.idx)
    assert torch.equal(whole.val, g.val) and torch.equal(whole.node_ids.long(), torch.arange(n))
    # an int is random_partition(num_nodes, P, seed)
    loader = mk.ClusterLoader(g, 5, seed=3)
    assert torch.equal(loader.parts, mk.random_partition(n, 5, 3)) and len(loader) == 5
    # cache=False builds anew
    loader = mk.ClusterLoader(g, parts, cache=False)
    a, b = list(loader), list(loader)
    assert all(x is not y and torch.equal(x.eids, y.eids) for x, y in zip(a, b))


def test_cluster_loader_shuffle_rule(host_loader):
    g = cpu_graph()
    parts = mk.random_partition(g.num_nodes, 6, 1)
    loader = mk.ClusterLoader(g, parts, clusters_per_batch=2, shuffle=True, seed=9)
    assert not loader.cache and len(loader) == 3
    for epoch in range(3):
        order = torch.randperm(6, generator=torch.Generator().manual_seed(
            mk.layer_seed(9, epoch, 0))).tolist()
        want = [tuple(sorted(order[b:b + 2])) for b in (0, 2, 4)]
        assert loader.batches(epoch) == want
        assert loader.epoch == epoch
        subs = list(loader)
        for sub, clusters in zip(subs, want):
            nodes = torch.nonzero(torch.isin(parts, torch.tensor(clusters))).flatten()
            assert torch.equal(sub.node_ids.long(), nodes)
    assert len({tuple(loader.batches(e)) for e in range(6)}) > 1      # redrawn per epoch
    assert not loader._subgraphs                                      # nothing is kept
    # one cluster per batch: the subgraphs recur in another order, so they are kept
    single = mk.ClusterLoader(g, parts, shuffle=True, seed=9)
    assert single.cache
    a = {tuple(s.node_ids.tolist()): s for s in single}
    b = {tuple(s.node_ids.tolist()): s for s in single}
    assert a.keys() == b.keys() and all(a[k] is b[k] for k in a)
    # without shuffle the batches do not depend on the epoch
    fixed = mk.ClusterLoader(g, parts, clusters_per_batch=2)
    assert fixed.batches(0) == fixed.batches(5) == [(0, 1), (2, 3), (4, 5)]


def test_subgraph_invariants():
    g = cpu_graph()
    nodes = torch.from_numpy(sg.node_sets()["half"].copy())
    sub = node_subgraph_on_the_host(g, nodes)
    out_ptr, col, eid, _ = sg.reference("half")
    assert isinstance(sub, mk.CSRGraph) and not isinstance(sub, mk.Block)
    assert sub.num_nodes == nodes.numel() and sub.num_edges == col.size
    assert sub.parent_num_nodes == g.num_nodes
    assert sub.ptr.dtype == sub.idx.dtype == sub.eids.dtype == sub.node_ids.dtype == torch.int32
    assert torch.equal(sub.val, g.val[sub.eids.long()])
    w = torch.rand(g.num_edges, 3)
    assert torch.equal(sub.edge_data(w), w[sub.eids.long()])
    assert torch.equal(sub.node_ids[sub.idx.long()].long(), g.idx[sub.eids.long()].long())
    # degrees and values over the subgraph's own edges
    assert sub.in_degrees().tolist() == np.diff(out_ptr).tolist()
    assert sub.out_degrees().tolist() == np.bincount(col, minlength=nodes.numel()).tolist()
    for kind in ("mean", "both", "sum"):
        want = sg.degree_values(out_ptr, col, kind)
        assert torch.allclose(sub.edge_values(kind).double(), want, rtol=1e-6), kind
        m = sub.with_values(kind)
        assert isinstance(m, mk.Subgraph) and m is sub.with_values(kind)
        assert m.ptr is sub.ptr and m.idx is sub.idx and m.eids is sub.eids
        assert m.node_ids is sub.node_ids and m.parent_num_nodes == sub.parent_num_nodes
        assert torch.equal(m.val, sub.edge_values(kind))
    ptr_t, idx_t, order = sub.transposed_structure()
    want_t = sg.gh.transposed(out_ptr, col, nodes.numel())
    assert np.array_equal(ptr_t.numpy(), want_t[0]) and np.array_equal(idx_t.numpy(), want_t[1])
    assert np.array_equal(order.numpy(), want_t[2])
    # the plans live on the object, as a Block's do, not in the global cache
    assert mk.Subgraph.plan is not mk.CSRGraph.plan
    # nothing changes for a plain CSRGraph
    assert type(g.with_values("mean")) is mk.CSRGraph and not hasattr(g, "eids")


# ------------------------------------------------------------------ selectors, fixtures
def test_restated_names_cover_the_fixture():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_sg::") for n in names)
    assert set(sg.KERNELS) == set(names) | set(sg.SCAN_KERNELS) and len(names) == 4
    assert all(n.startswith("maxk_scan::") for n in sg.SCAN_KERNELS)
    assert set(sg.COUNT_KERNELS) | set(sg.FILL_KERNELS) == set(sg.KERNELS)


def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_sg::") == kernel_list.read_list(FIXTURE)
    assert kernel_list.main([_lib.LIB_PATH, "--namespace", "maxk_sg::", "--diff", FIXTURE]) == 0
