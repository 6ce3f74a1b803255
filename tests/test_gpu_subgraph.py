"""GPU: maxk_induced_subgraph_count / _fill against the numpy restatement of tests/subgraph.py,
bit for bit (the rule is part of the ABI); their output contract on guarded, poisoned buffers;
capture; every layer on the identity subgraph against the full graph, bit for bit, and on a random
half against float64; edge_weight through Subgraph.edge_data; and a MaxKGCN trained over
ClusterLoader with cached subgraphs and plans. The graph is the 600-row one of the multi-head
tests (hub row 5,000, hub column 3,000); tests/test_subgraph_capi.py checks the preconditions of
the node sets. The count's scan runs at the lengths of tests/scan.py. The last test closes over the
compiled maxk_sg:: instantiations and the maxk_scan:: kernels the count launches.

Worst norm-wise differences print with -s."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import maxk_kernels as mk
import scan
import subgraph as sg
from arena import POISONS, arena
from maxk_kernels import _lib, ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations_subgraph.txt")
COVERED = set()      # kernel names launched by a case that went on to pass
P = ctypes.c_void_p
lib = _lib.lib


def dev_of(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)      # a copy: the cached arrays are read-only


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape,
                                                                 got.dtype, want.dtype)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def compiled():
    """The maxk_sg:: fixture and the maxk_scan:: kernels the count launches."""
    with open(FIXTURE) as f:
        return {ln.strip() for ln in f if ln.strip()} | set(sg.SCAN_KERNELS)


@functools.lru_cache(maxsize=None)
def graph_dev(dev):
    ptr, idx, _ = sg.graph()
    return dev_of(ptr, dev), dev_of(idx, dev)


def csr_graph(dev, val=None):
    ptr, idx = graph_dev(dev)
    return mk.CSRGraph(ptr, idx, val)


def extract(ptr_d, idx_d, nodes, dev):
    """(out_ptr, out_col, out_eid, counts) as numpy through ops: count, read M back, fill."""
    nodes_d = dev_of(np.asarray(nodes, np.int32), dev)
    out_ptr, counts = ops.induced_subgraph_count(ptr_d, idx_d, nodes_d)
    counts = tuple(int(v) for v in counts.tolist())
    col, eid = ops.induced_subgraph_fill(ptr_d, idx_d, nodes_d, out_ptr, capacity=counts[0])
    return out_ptr.cpu().numpy(), col.cpu().numpy(), eid.cpu().numpy(), counts


def check_against(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("out_ptr", "out_col", "out_eid")):
        same(g, w, f"{what}: {name}")
    assert got[3] == want[3], (what, got[3], want[3])


def test_limits_are_the_restated_ones(gpu):
    assert ops.subgraph_row_limits() == sg.LIMITS


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name", sorted(sg.node_sets()))
def test_extraction_matches_the_restatement_bit_for_bit(gpu, name):
    ptr_d, idx_d = graph_dev(gpu)
    nodes = sg.node_sets()[name]
    check_against(extract(ptr_d, idx_d, nodes, gpu), sg.reference(name), name)
    if nodes.size:
        COVERED.update(sg.KERNELS)


def test_idx_that_starts_off_a_16_byte_boundary(gpu):
    """The rows are read as aligned quads counted from idx's own address: the same result when
    idx starts 4, 8 or 12 bytes off a 16-byte boundary."""
    ptr, idx, _ = sg.graph()
    ptr_d, _ = graph_dev(gpu)
    for shift in (1, 2, 3):
        buf = torch.zeros(idx.size + 8, dtype=torch.int32, device=gpu)
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + idx.size]
        view.copy_(dev_of(idx, gpu))
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        for name in ("half", "every_column", "hub", "permuted"):
            check_against(extract(ptr_d, view, sg.node_sets()[name], gpu), sg.reference(name),
                          f"{name}, idx shifted by {shift}")


def test_a_rows_output_does_not_depend_on_the_order_of_the_selection(gpu):
    """The same set in three orders: every row keeps the same parent edges, and the same columns
    once the local numbers are mapped back through nodes."""
    ptr_d, idx_d = graph_dev(gpu)
    base = sg.node_sets()["few_columns"].astype(np.int64)
    rng = np.random.default_rng(5)
    a_ptr, a_col, a_eid, _ = extract(ptr_d, idx_d, base, gpu)
    for order in (base[::-1].copy(), rng.permutation(base), np.sort(base)):
        o_ptr, o_col, o_eid, counts = extract(ptr_d, idx_d, order, gpu)
        assert counts == (a_eid.size, base.size, 0)
        where = {int(r): i for i, r in enumerate(order)}
        for i, r in enumerate(base):
            j = where[int(r)]
            mine, theirs = slice(a_ptr[i], a_ptr[i + 1]), slice(o_ptr[j], o_ptr[j + 1])
            same(o_eid[theirs], a_eid[mine], f"row {r}: eids")
            same(order[o_col[theirs]], base[a_col[mine]], f"row {r}: columns, relabelled")


def test_repeated_and_out_of_range_nodes(gpu):
    ptr, idx, n = sg.graph()
    ptr_d, idx_d = graph_dev(gpu)
    graph = csr_graph(gpu)
    repeated = np.array([30, 40, 30, sg.HUB, 50, 40, 580], np.int32)
    stray = np.array([30, n, -3, sg.HUB, 50, 2 ** 31 - 1, -2 ** 31], np.int32)
    for nodes, counts in ((repeated, (5, 0)), (stray, (5, 4))):
        want = sg.subgraph_ref(ptr, idx, nodes, n)
        assert want[3][1:] == counts
        check_against(extract(ptr_d, idx_d, nodes, gpu), want, str(nodes.tolist()))
    with pytest.raises(ValueError, match="nodes must be distinct: 7 entries name 5 nodes"):
        mk.node_subgraph(graph, dev_of(repeated, gpu))
    with pytest.raises(ValueError, match=rf"4 of the 7 nodes lie outside \[0, {n}\)"):
        mk.node_subgraph(graph, dev_of(stray, gpu))
    # an int64 id that would wrap into [0, n) when narrowed to int32 is still out of range
    wide = torch.tensor([30, 2 ** 32 + 5, 50, -2 ** 40], dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError, match=rf"2 of the 4 nodes lie outside \[0, {n}\)"):
        mk.node_subgraph(graph, wide)
    ok = mk.node_subgraph(graph, torch.tensor([30, 5, 50], dtype=torch.int64, device=gpu))
    assert ok.node_ids.dtype == torch.int32 and ok.node_ids.tolist() == [30, 5, 50]
    COVERED.update(sg.KERNELS)


def test_node_subgraph_is_the_restated_subgraph(gpu):
    ptr, idx, n = sg.graph()
    val = np.random.default_rng(2).random(idx.size).astype(np.float32)
    graph = csr_graph(gpu, dev_of(val, gpu))
    for name in ("half", "permuted", "none", "hub"):
        nodes = sg.node_sets()[name]
        sub = mk.node_subgraph(graph, dev_of(nodes, gpu))
        out_ptr, col, eid, _ = sg.reference(name)
        assert isinstance(sub, mk.Subgraph) and sub.parent_num_nodes == n
        same(sub.ptr.cpu().numpy(), out_ptr, "ptr")
        same(sub.idx.cpu().numpy(), col, "idx")
        same(sub.eids.cpu().numpy(), eid, "eids")
        same(sub.node_ids.cpu().numpy(), nodes, "node_ids")
        same(sub.val.cpu().numpy(), val[eid], "val")
        assert sub.num_edges == eid.size        # exactly M entries
    with pytest.raises(TypeError, match="rectangular"):
        mk.node_subgraph(mk.Block(graph.ptr, graph.idx, num_src=n), dev_of(nodes, gpu))
    # the plans live on the object: one per (D, k), rebuilt after an in-place edit of the
    # structure that the version counter shows, as ops.get_plan's key would
    sub = mk.node_subgraph(graph, dev_of(sg.node_sets()["half"], gpu))
    plan = sub.plan(64, 8)
    assert sub.plan(64, 8) is plan and sub.plan(64, 16) is not plan
    assert plan not in ops._PLAN_CACHE.values()
    sub.idx.add_(0)
    assert sub.plan(64, 8) is not plan


# ------------------------------------------------------------------ 2. output contract
def raw_count(ptr_d, idx_d, nodes_d, a_ptr, a_cnt, a_scr, n, e):
    return lib.maxk_induced_subgraph_count(P(ptr_d.data_ptr()), P(idx_d.data_ptr()),
                                           P(nodes_d.data_ptr()), P(a_ptr.ptr), P(a_cnt.ptr),
                                           P(a_scr.ptr), a_scr.nbytes, n, e, nodes_d.numel(), None)


def raw_fill(ptr_d, idx_d, nodes_d, out_ptr, a_col, a_eid, cap, a_scr, n, e):
    return lib.maxk_induced_subgraph_fill(P(ptr_d.data_ptr()), P(idx_d.data_ptr()),
                                          P(nodes_d.data_ptr()), P(out_ptr), P(a_col.ptr),
                                          P(a_eid.ptr), cap, P(a_scr.ptr), a_scr.nbytes, n, e,
                                          nodes_d.numel(), None)


@pytest.mark.parametrize("poison", POISONS)
def test_output_contract(gpu, poison):
    """Poisoned outputs are fully written in their defined ranges, nothing is written past M,
    the bound or the reported scratch size, and scratch that arrives dirty (both poisons, for
    both calls) changes no output. A bound below M cuts the output and writes nothing past it."""
    ptr, idx, n = sg.graph()
    ptr_d, idx_d = graph_dev(gpu)
    poison32 = np.frombuffer(bytes([poison] * 4), np.int32)[0]
    for name in ("half", "few_columns", "every_column", "hub"):
        nodes = sg.node_sets()[name]
        w_ptr, w_col, w_eid, w_counts = sg.reference(name)
        s, m = nodes.size, w_counts[0]
        nodes_d = dev_of(nodes, gpu)
        sb = ops.induced_subgraph_scratch_bytes(n, s)
        assert sb == sg.scratch_bytes(n, s)
        a_ptr = arena((1, s + 1, torch.int32), gpu, poison)
        a_cnt = arena((1, 3, torch.int32), gpu, poison)
        a_scr = arena(sb, gpu, poison)
        assert raw_count(ptr_d, idx_d, nodes_d, a_ptr, a_cnt, a_scr, n, idx.size) == 0
        torch.cuda.synchronize()
        for a, what in ((a_ptr, "out_ptr"), (a_cnt, "counts"), (a_scr, "scratch")):
            assert a.check() is None, (name, what, a.check())
        same(a_ptr.payload.cpu().numpy()[0], w_ptr, f"{name}: out_ptr in the arena")
        assert tuple(a_cnt.payload.cpu().numpy()[0].tolist()) == w_counts
        for cap in (m + 100, m, m // 2, 0):
            a_col, a_eid = (arena((1, cap, torch.int32), gpu, poison) for _ in range(2))
            a_scr = arena(sb, gpu, poison)
            assert raw_fill(ptr_d, idx_d, nodes_d, a_ptr.ptr, a_col, a_eid, cap, a_scr, n,
                            idx.size) == 0
            torch.cuda.synchronize()
            for a, what in ((a_col, "out_col"), (a_eid, "out_eid"), (a_scr, "scratch"),
                            (a_ptr, "out_ptr")):
                assert a.check() is None, (name, cap, what, a.check())
            same(a_ptr.payload.cpu().numpy()[0], w_ptr, "out_ptr after the fill")
            for a, want, what in ((a_col, w_col, "out_col"), (a_eid, w_eid, "out_eid")):
                got = a.payload.cpu().numpy()[0]
                same(got[:min(m, cap)], want[:cap], f"{name} bound {cap}: {what}")
                assert (got[m:] == poison32).all(), f"{name} bound {cap}: {what} written past M"
    COVERED.update(sg.KERNELS)


def test_zero_sizes(gpu):
    ptr, idx, n = sg.graph()
    ptr_d, idx_d = graph_dev(gpu)
    # no nodes: out_ptr[0] = 0 and counts = {0, 0, 0}, nothing else
    none = torch.zeros(0, dtype=torch.int32, device=gpu)
    a_ptr, a_cnt = arena((1, 1, torch.int32), gpu, 0xFF), arena((1, 3, torch.int32), gpu, 0xFF)
    a_scr = arena(ops.induced_subgraph_scratch_bytes(n, 0), gpu, 0xFF)
    assert raw_count(ptr_d, idx_d, none, a_ptr, a_cnt, a_scr, n, idx.size) == 0
    a_col, a_eid = (arena((1, 8, torch.int32), gpu, 0xFF) for _ in range(2))
    assert raw_fill(ptr_d, idx_d, none, a_ptr.ptr, a_col, a_eid, 8, a_scr, n, idx.size) == 0
    torch.cuda.synchronize()
    assert a_ptr.payload.tolist() == [[0]] and a_cnt.payload.tolist() == [[0, 0, 0]]
    for a in (a_ptr, a_cnt, a_scr, a_col, a_eid):
        assert a.check() is None
    assert (a_col.payload == -1).all() and (a_eid.payload == -1).all()
    assert (a_scr.payload == 0xFF).all()
    # no edges: zeros
    empty_ptr = torch.zeros(n + 1, dtype=torch.int32, device=gpu)
    empty_idx = torch.zeros(0, dtype=torch.int32, device=gpu)
    nodes = sg.node_sets()["half"]
    got = extract(empty_ptr, empty_idx, nodes, gpu)
    same(got[0], np.zeros(nodes.size + 1, np.int32), "out_ptr without edges")
    assert got[1].size == 0 == got[2].size and got[3] == (0, nodes.size, 0)
    sub = mk.node_subgraph(mk.CSRGraph(empty_ptr, empty_idx), dev_of(nodes, gpu))
    assert sub.num_edges == 0 and sub.num_nodes == nodes.size


# ------------------------------------------------------------------ 3. capture
def test_both_calls_replay_from_one_captured_graph(gpu):
    ptr, idx, n = sg.graph()
    ptr_d, idx_d = graph_dev(gpu)
    base = sg.node_sets()["half"]
    sets = [base, base[::-1].copy(), np.roll(base, 7)]       # one set: one edge count
    refs = [sg.subgraph_ref(ptr, idx, s, n) for s in sets]
    m, s = refs[0][3][0], base.size
    assert all(r[3][0] == m for r in refs) and not np.array_equal(refs[0][2], refs[1][2])
    nodes_d = dev_of(sets[0], gpu)
    out = (torch.empty(s + 1, dtype=torch.int32, device=gpu),
           torch.empty(3, dtype=torch.int32, device=gpu))
    fout = (torch.empty(m, dtype=torch.int32, device=gpu),
            torch.empty(m, dtype=torch.int32, device=gpu))
    scratch = torch.empty(ops.induced_subgraph_scratch_bytes(n, s), dtype=torch.uint8, device=gpu)

    def step():
        ops.induced_subgraph_count(ptr_d, idx_d, nodes_d, out=out, scratch=scratch)
        ops.induced_subgraph_fill(ptr_d, idx_d, nodes_d, out[0], out=fout, scratch=scratch)

    step()                                     # eager once: equal to the restatement
    torch.cuda.synchronize()
    same(fout[1].cpu().numpy(), refs[0][2], "eager out_eid")
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        step()
    for which in (1, 2, 0, 1):
        nodes_d.copy_(dev_of(sets[which], gpu))
        for t in out + fout:
            t.fill_(-7)
        scratch.fill_(0x5A)
        cg.replay()
        torch.cuda.synchronize()
        got = (out[0].cpu().numpy(), fout[0].cpu().numpy(), fout[1].cpu().numpy(),
               tuple(out[1].tolist()))
        check_against(got, refs[which], f"replay {which}")
    COVERED.update(sg.KERNELS)


# ------------------------------------------------------------------ 4. layers
FIN, FOUT, K = 64, 48, 8
LAYERS = ("sage_mean", "sage_pool", "sage_gcn", "gcn", "gin", "gat1", "gat4")


def make_layer(kind, dev):
    torch.manual_seed(LAYERS.index(kind) + 11)
    if kind.startswith("sage_"):
        layer = mk.MaxKSAGEConv(FIN, FOUT, kind[5:], maxk=K)
    elif kind == "gcn":
        layer = mk.MaxKGCNConv(FIN, FOUT, maxk=K, allow_zero_in_degree=True)
    elif kind == "gin":
        layer = mk.MaxKGINConv(FIN, maxk=K, init_eps=0.3)
    else:
        heads = int(kind[3:])
        layer = mk.MaxKGATConv(FIN, 64 // heads, maxk=K, num_heads=heads,
                               allow_zero_in_degree=True)
    layer = layer.to(dev)
    with torch.no_grad():
        if getattr(layer, "bias", None) is not None:
            layer.bias.normal_()
    return layer


def rel(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp(min=1e-300))


@pytest.mark.parametrize("kind", LAYERS)
def test_identity_subgraph_gives_the_full_graphs_output_bit_for_bit(gpu, kind):
    graph = csr_graph(gpu)
    n = graph.num_nodes
    sub = mk.node_subgraph(graph, torch.arange(n, dtype=torch.int32, device=gpu))
    assert torch.equal(sub.ptr, graph.ptr) and torch.equal(sub.idx, graph.idx)
    assert torch.equal(sub.eids, torch.arange(graph.num_edges, dtype=torch.int32, device=gpu))
    assert torch.equal(sub.val, graph.val)
    layer = make_layer(kind, gpu)
    x = torch.randn(n, FIN, device=gpu)
    with torch.no_grad():
        want, got = layer(graph, x), layer(sub, x)
    assert got.shape == want.shape and torch.equal(got, want), rel(got, want)
    COVERED.update(sg.KERNELS)


def given_for(kind, layer, sub, feat):
    """What is discrete in the f32 run, for the float64 restatement."""
    with torch.no_grad():
        if kind == "gcn":
            return {"sel": mk.maxk(feat @ layer.weight, K)[1]}
        if kind.startswith("gat"):
            return {"sel": mk.maxk(layer.fc(feat), K)[1]}
        sp_data, sel = mk.maxk(feat, K)
        given = {"sel": sel}
        if kind == "sage_pool":
            pd, sel2 = mk.maxk(layer.fc_pool(mk.densify(sp_data, sel, FIN)), K)
            _, arg_edge, _ = mk.max_aggregate(sub, pd, sel2, FIN, return_arg=True)
            given.update(sel_pool=sel2, arg_edge=arg_edge)
        return given


@pytest.mark.parametrize("kind", LAYERS)
def test_layers_on_a_random_half_against_float64(gpu, kind):
    """Forward and parameter gradients on A[nodes][:, nodes] with the subgraph's own degrees,
    1e-5 norm-wise (the layers' tolerance)."""
    graph = csr_graph(gpu)
    nodes = sg.node_sets()["half"]
    sub = mk.node_subgraph(graph, dev_of(nodes, gpu))
    sptr, scol, _, _ = sg.reference("half")
    layer = make_layer(kind, gpu)
    feats = torch.randn(graph.num_nodes, FIN, device=gpu)
    x = feats[sub.node_ids.long()]
    out = layer(sub, x)
    probe = torch.randn_like(out)
    (out * probe).sum().backward()
    ref_kind = "gat" if kind.startswith("gat") else kind
    ref, p, _ = sg.layer64(ref_kind, layer, sptr, scol, x, given_for(kind, layer, sub, x))
    (ref * probe.double().cpu()).sum().backward()
    worst = [("output", rel(out, ref))]
    worst += [(name, rel(v.grad, p[name].grad)) for name, v in layer.named_parameters()]
    print(f"\n  {kind}: " + ", ".join(f"{n} {e:.2e}" for n, e in worst))
    assert out.shape == ref.shape
    for name, e in worst:
        assert e <= 1e-5, (kind, name, e)


def test_edge_weight_through_edge_data(gpu):
    graph = csr_graph(gpu)
    nodes = sg.node_sets()["half"]
    sub = mk.node_subgraph(graph, dev_of(nodes, gpu))
    sptr, scol, seid, _ = sg.reference("half")
    layer = make_layer("gcn", gpu)
    x = torch.randn(nodes.size, FIN, device=gpu)
    w = (torch.rand(graph.num_edges, device=gpu) + 0.5).requires_grad_(True)
    ew = sub.edge_data(w)
    assert ew.shape == (seid.size,) and torch.equal(ew.detach(), w.detach()[sub.eids.long()])
    out = layer(sub, x, edge_weight=ew)
    probe = torch.randn_like(out)
    (out * probe).sum().backward()
    ref, p, w64 = sg.layer64("gcn", layer, sptr, scol, x, given_for("gcn", layer, sub, x),
                             edge_weight=ew)
    (ref * probe.double().cpu()).sum().backward()
    assert rel(out, ref) <= 1e-5, rel(out, ref)
    for name, v in layer.named_parameters():
        assert rel(v.grad, p[name].grad) <= 1e-5, (name, rel(v.grad, p[name].grad))
    eids = torch.from_numpy(seid.astype(np.int64))
    got = w.grad.cpu()
    assert rel(got[eids], w64.grad) <= 1e-5, rel(got[eids], w64.grad)
    rest = torch.ones(graph.num_edges, dtype=torch.bool)
    rest[eids] = False
    assert rest.any() and not got[rest].any()       # edges outside the subgraph: no gradient


# ------------------------------------------------------------------ 5. cluster mini-batches
def gcn_model64(model, sptr, scol, x, sels):
    """MaxKGCN (norm=False, eval of dropout: feat_drop = 0) in float64 with the selections
    given: (logits, parameters)."""
    p = {n: v.detach().double().cpu().requires_grad_(True) for n, v in model.named_parameters()}
    values = sg.degree_values(sptr, scol, "both")
    h = torch.relu(x.detach().double().cpu() @ p["lin_in.weight"].t() + p["lin_in.bias"])
    for i, sel in enumerate(sels):
        h = h @ p[f"linlayers.{i}.weight"].t() + p[f"linlayers.{i}.bias"]
        h = sg.aggregate64(sptr, scol, values, sg.masked64(h, sel.cpu().long()))
        h = h + p[f"gcnlayers.{i}.bias"]
    return h @ p["lin_out.weight"].t() + p["lin_out.bias"], p


def test_two_layer_gcn_trains_over_the_cluster_loader(gpu, monkeypatch):
    ptr, idx, n = sg.graph()
    graph = csr_graph(gpu)
    created = []
    for name in [s for s in _lib.SIGNATURES if s.startswith("maxk_plan_create")]:
        def counting(*args, _real=getattr(lib, name), _name=name):
            created.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    mk.clear_plan_cache()
    loader = mk.ClusterLoader(graph, 4, seed=1)
    parts = mk.random_partition(n, 4, 1)
    assert len(loader) == 4 and torch.equal(loader.parts, parts)
    fin, hid, classes = 32, 64, 5
    torch.manual_seed(21)
    model = mk.MaxKGCN(fin, hid, 2, classes, maxk=K, feat_drop=0.0).to(gpu)
    with torch.no_grad():
        for conv in model.gcnlayers:
            conv.bias.normal_()
    feats = torch.randn(n, fin, device=gpu)
    labels = torch.randint(0, classes, (n,), device=gpu)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    seen = []
    hooks = [conv.register_forward_pre_hook(lambda mod, args: seen.append(args[1].detach()))
             for conv in model.gcnlayers]
    first = []
    for b, sub in enumerate(loader):
        ids = sub.node_ids.long()
        want_ids = torch.nonzero(parts == b).flatten()
        assert torch.equal(ids.cpu(), want_ids)
        sref = sg.subgraph_ref(ptr, idx, want_ids.numpy(), n)
        same(sub.ptr.cpu().numpy(), sref[0], f"batch {b}: ptr")
        same(sub.idx.cpu().numpy(), sref[1], f"batch {b}: idx")
        del seen[:]
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(sub, feats[ids]), labels[ids])
        loss.backward()
        sels = [mk.maxk(s, K)[1] for s in seen]
        assert len(sels) == 2
        logits, p = gcn_model64(model, sref[0], sref[1], feats[ids], sels)
        loss64 = torch.nn.functional.cross_entropy(logits, labels[ids].cpu())
        loss64.backward()
        worst = [("loss", rel(loss, loss64))]
        worst += [(name, rel(v.grad, p[name].grad)) for name, v in model.named_parameters()]
        print(f"\n  batch {b}: " + ", ".join(f"{a} {e:.1e}" for a, e in worst))
        for name, e in worst:
            assert e <= 1e-5, (b, name, e)
        opt.step()
        first.append(sub)
    for h in hooks:
        h.remove()
    built = len(created)
    assert built >= 4                               # a plan per cluster at least
    assert not ops._PLAN_CACHE                      # and none of them in the global cache
    second = []
    for sub in loader:                              # the second epoch
        ids = sub.node_ids.long()
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(sub, feats[ids]), labels[ids]).backward()
        opt.step()
        second.append(sub)
    assert len(second) == 4 and all(a is b for a, b in zip(first, second))
    assert len(created) == built, created[built:]   # no plan was rebuilt
    mk.clear_plan_cache()
    COVERED.update(sg.KERNELS)


# ------------------------------------------------------------------ 6. scan lengths
@pytest.mark.parametrize("n", scan.LENGTHS)
def test_count_scans_n_items(gpu, n):
    """out_ptr is scanned over S + 1 = n items: S positions drawn with repetition from the 600
    nodes, the last three of them (the last tile of the positions) out of range. counts holds the
    kept edges, the distinct nodes and the entries out of range."""
    ptr, idx, num = sg.graph()
    ptr_d, idx_d = graph_dev(gpu)
    nodes = np.random.default_rng(n).integers(0, num, n - 1).astype(np.int32)
    nodes[max(n - 4, 0):] = (num, -1, 2 ** 31 - 1)[:min(3, n - 1)]
    w_ptr, w_counts = sg.count_ref(ptr, idx, nodes, num)
    assert w_counts[2] == min(3, n - 1) and w_counts[0] < 2 ** 31
    out_ptr, counts = ops.induced_subgraph_count(ptr_d, idx_d, dev_of(nodes, gpu))
    same(out_ptr.cpu().numpy(), w_ptr, f"{n} items: out_ptr")
    assert tuple(counts.tolist()) == w_counts, (n, counts.tolist(), w_counts)
    if nodes.size:
        COVERED.update(sg.COUNT_KERNELS)


# ------------------------------------------------------------------ 7. closure (keep last)
def test_every_subgraph_instantiation_was_launched_by_a_passing_case(gpu):
    names = compiled()
    assert len(names) == 4 + len(sg.SCAN_KERNELS) == 7
    missing = sorted(names - COVERED)
    assert not missing, f"instantiations without a passing case: {missing}"
    assert not COVERED - names
