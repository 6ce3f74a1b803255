"""GPU: maxk_csr_transpose against the numpy restatement of tests/transpose.py, bit for bit in all
four outputs (the rule is part of the ABI); its output contract on guarded, poisoned buffers;
capture; the wiring of CSRGraph, Block and Subgraph against the torch path they had before; the
registered operator; and one backward per consumer of A^T, bit-equal between a graph whose
structure the kernel built and a twin whose structure the torch path built. tests/
test_transpose_capi.py checks the preconditions of the cases. Both scans run at the lengths of
tests/scan.py. The last test closes over the compiled maxk_tr:: instantiations and the maxk_scan::
kernels of the plain scan."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import maxk_kernels as mk
import scan
import subgraph as sg
import transpose as tr
from arena import POISONS, arena
from maxk_kernels import _lib, autograd, ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations_transpose.txt")
COVERED = set()      # kernel names launched by a case that went on to pass
P = ctypes.c_void_p
lib = _lib.lib
NAMES = ("out_ptr", "out_row", "out_order", "out_val")


def dev_of(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)      # a copy: the cached arrays are read-only


def bits_of(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    got, want = bits_of(got), bits_of(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape,
                                                                 got.dtype, want.dtype)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def compiled():
    """The maxk_tr:: fixture and the maxk_scan:: kernels a call launches."""
    with open(FIXTURE) as f:
        return {ln.strip() for ln in f if ln.strip()} | set(tr.SCAN_KERNELS)


def run_case(ptr, idx, nc, dev, what, idx_d=None):
    """ops.csr_transpose with and without values against the restatement."""
    ptr_d = dev_of(ptr, dev)
    idx_d = dev_of(idx, dev) if idx_d is None else idx_d
    val = tr.values(idx.size, idx.size % 13)
    want = tr.transpose_ref(ptr, idx, nc, val)
    for v in (None, dev_of(val, dev)):
        got = ops.csr_transpose(ptr_d, idx_d, v, nc)
        assert len(got) == (3 if v is None else 4)
        for g, w, name in zip(got, want, NAMES):
            assert g.device == ptr_d.device
            same(g.cpu().numpy(), w, f"{what}: {name}{'' if v is None else ' (with val)'}")
        if idx.size:
            COVERED.update(tr.kernels(nc, v is not None))


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name", sorted(tr.cases()))
def test_transposition_matches_the_restatement_bit_for_bit(gpu, name):
    ptr, idx, nc = tr.cases()[name]
    run_case(ptr, idx, nc, gpu, name)


@pytest.mark.parametrize("nc", tr.column_counts())
def test_every_digit_plan(gpu, nc):
    """About 3,000 edges over num_cols columns, on both sides of every digit boundary. The largest
    case, 2^22 + 1 columns, has an out_ptr of 4 * (2^22 + 2) bytes = 16 MiB."""
    assert 4 * (nc + 1) <= 128 << 20
    assert ops.transpose_digit_bits(nc) == tr.digit_bits(nc)
    ptr, idx, _ = tr.plan_case(nc)
    run_case(ptr, idx, nc, gpu, f"{nc} columns")


def test_no_columns_and_no_edges(gpu):
    empty = torch.zeros(0, dtype=torch.int32, device=gpu)
    for n, nc in ((0, 0), (5, 0), (0, 7)):
        got = ops.csr_transpose(torch.zeros(n + 1, dtype=torch.int32, device=gpu), empty, None, nc)
        assert got[0].tolist() == [0] * (nc + 1) and got[1].numel() == 0 == got[2].numel()


def test_idx_that_starts_off_a_16_byte_boundary(gpu):
    for name in ("square", "edges_8193"):
        ptr, idx, nc = tr.cases()[name]
        for shift in (1, 2, 3):
            buf = torch.zeros(idx.size + 8, dtype=torch.int32, device=gpu)
            assert buf.data_ptr() % 16 == 0
            view = buf[shift:shift + idx.size]
            view.copy_(dev_of(idx, gpu))
            assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
            run_case(ptr, idx, nc, gpu, f"{name}, idx shifted by {shift}", idx_d=view)


# ------------------------------------------------------------------ 2. output contract
def raw(ptr_d, idx_d, val_d, arenas, scr, n, nc, e):
    a_ptr, a_row, a_order, a_val = arenas
    return lib.maxk_csr_transpose(P(ptr_d.data_ptr()), P(idx_d.data_ptr()),
                                  P(val_d.data_ptr()) if val_d is not None else None,
                                  P(a_ptr.ptr), P(a_row.ptr), P(a_order.ptr),
                                  P(a_val.ptr) if val_d is not None else None, P(scr.ptr),
                                  scr.nbytes, n, nc, e, None)


CONTRACT_CASES = ("square", "rect_t", "one_column", "edges_8191", "stray_columns", "plan_3")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", CONTRACT_CASES)
def test_output_contract(gpu, name, poison):
    """Poisoned outputs are fully written and nothing is written around them or around scratch of
    exactly the reported size, which arrives dirty; without val, out_val is not touched."""
    ptr, idx, nc = tr.plan_case(2 ** 22 + 1) if name == "plan_3" else tr.cases()[name]
    n, e = ptr.size - 1, idx.size
    val = tr.values(e, 5)
    want = tr.transpose_ref(ptr, idx, nc, val)
    ptr_d, idx_d, val_d = dev_of(ptr, gpu), dev_of(idx, gpu), dev_of(val, gpu)
    sb = ops.csr_transpose_scratch_bytes(n, nc, e)
    assert sb == tr.scratch_bytes(n, nc, e)
    for v in (val_d, None):
        arenas = (arena((1, nc + 1, torch.int32), gpu, poison),
                  arena((1, e, torch.int32), gpu, poison), arena((1, e, torch.int32), gpu, poison),
                  arena((1, e, torch.float32), gpu, poison))
        scr = arena(sb, gpu, poison)
        assert raw(ptr_d, idx_d, v, arenas, scr, n, nc, e) == 0, lib.maxk_last_error()
        torch.cuda.synchronize()
        for a, what in zip(arenas + (scr,), NAMES + ("scratch",)):
            assert a.check() is None, (name, what, a.check())
        for a, w, what in zip(arenas[:3], want, NAMES):
            assert a.first_poisoned() is None, (name, what, a.first_poisoned())
            same(a.payload.cpu().numpy()[0], w, f"{name}: {what} in the arena")
        got_val = arenas[3].payload.cpu().numpy()[0]
        if v is None:
            assert (got_val.view(np.uint8) == poison).all(), "out_val written without val"
        else:
            same(got_val, want[3], f"{name}: out_val in the arena")
        COVERED.update(tr.kernels(nc, v is not None))


def test_no_edges_writes_out_ptr_alone(gpu):
    for nc in (0, 40):
        a_ptr = arena((1, nc + 1, torch.int32), gpu, 0xFF)
        rest = tuple(arena((1, 8, torch.int32), gpu, 0xFF) for _ in range(2)) + \
            (arena((1, 8, torch.float32), gpu, 0xFF),)
        scr = arena(64, gpu, 0xFF)
        ptr_d = torch.zeros(41, dtype=torch.int32, device=gpu)
        assert raw(ptr_d, ptr_d, ptr_d.float(), (a_ptr,) + rest, scr, 40, nc, 0) == 0
        torch.cuda.synchronize()
        assert a_ptr.payload.tolist() == [[0] * (nc + 1)]
        for a in (a_ptr, scr) + rest:
            assert a.check() is None
            assert a is a_ptr or (a.payload.view(torch.uint8) == 0xFF).all()


# ------------------------------------------------------------------ 3. capture
def test_replays_from_a_captured_graph(gpu):
    ptr, idx, nc = tr.cases()["square"]
    rng = np.random.default_rng(9)
    idxs = [idx, (idx.astype(np.int64) * 7 % nc).astype(np.int32), rng.permutation(idx)]
    vals = [tr.values(idx.size, s) for s in (1, 2, 3)]
    refs = [tr.transpose_ref(ptr, i, nc, v) for i, v in zip(idxs, vals)]
    assert not np.array_equal(refs[0][2], refs[1][2])
    e, n = idx.size, ptr.size - 1
    ptr_d, idx_d, val_d = dev_of(ptr, gpu), dev_of(idxs[0], gpu), dev_of(vals[0], gpu)
    out = (torch.empty(nc + 1, dtype=torch.int32, device=gpu),
           torch.empty(e, dtype=torch.int32, device=gpu),
           torch.empty(e, dtype=torch.int32, device=gpu),
           torch.empty(e, dtype=torch.float32, device=gpu))
    scratch = torch.empty(ops.csr_transpose_scratch_bytes(n, nc, e), dtype=torch.uint8, device=gpu)

    def step():
        ops.csr_transpose(ptr_d, idx_d, val_d, nc, out=out, scratch=scratch)

    step()                                     # eager once: equal to the restatement
    torch.cuda.synchronize()
    eager = [t.cpu().numpy().copy() for t in out]
    for g, w, name in zip(eager, refs[0], NAMES):
        same(g, w, f"eager {name}")
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        step()
    for which in (1, 2, 0, 1):
        idx_d.copy_(dev_of(idxs[which], gpu))
        val_d.copy_(dev_of(vals[which], gpu))
        for t in out[:3]:
            t.fill_(-7)
        out[3].fill_(float("nan"))
        scratch.fill_(0x5A)
        cg.replay()
        torch.cuda.synchronize()
        for t, w, name in zip(out, refs[which], NAMES):
            same(t.cpu().numpy(), w, f"replay {which}: {name}")
    COVERED.update(tr.kernels(nc, True))


# ------------------------------------------------------------------ 4. wiring
def torch_path(g):
    """(ptr_t int32, idx_t int32, order int64, val_t) of the torch helper on g's own tensors."""
    ptr_t, rows, order = autograd._torch_transpose(g.ptr, g.idx, g._num_cols())
    return ptr_t.to(torch.int32), rows[order].to(torch.int32).contiguous(), order, g.val[order]


@pytest.fixture
def counted(monkeypatch):
    calls = []
    real = ops.csr_transpose

    def counting(*args, **kw):
        calls.append(args)
        return real(*args, **kw)

    monkeypatch.setattr(ops, "csr_transpose", counting)
    return calls


def graphs_on(dev):
    ptr, idx, n = sg.graph()
    val = dev_of(np.random.default_rng(4).random(idx.size).astype(np.float32), dev)
    graph = mk.CSRGraph(dev_of(ptr, dev), dev_of(idx, dev), val)
    seeds = torch.arange(0, n, 3, dtype=torch.int32, device=dev)
    block = mk.to_block(graph, seeds, 10, 5)
    sub = mk.node_subgraph(graph, dev_of(sg.node_sets()["half"], dev))
    return {"graph": graph, "block": block, "subgraph": sub}


@pytest.mark.parametrize("kind", ["graph", "block", "subgraph"])
def test_graphs_on_the_gpu_use_the_kernel_and_equal_the_torch_path(gpu, counted, kind):
    g = graphs_on(gpu)[kind]
    assert g.num_edges > 1000
    want = torch_path(g)
    before = len(counted)
    st = g.transposed_structure()
    assert len(counted) == before + 1 and st is g.transposed_structure()
    order = g.transposed_order()
    assert order is g.transposed_order() and len(counted) == before + 1      # the kernel's own
    assert [t.dtype for t in st] == [torch.int32, torch.int32, torch.int64]
    assert order.dtype == torch.int32 and order.is_contiguous()
    for got, w in zip(st + (order,), want[:3] + (want[2].to(torch.int32),)):
        assert got.device == g.ptr.device and got.dtype == w.dtype and torch.equal(got, w)
    assert torch.equal(g.out_degrees(), torch.bincount(g.idx.long(), minlength=g._num_cols()))
    shared = g.with_values("mean")
    assert type(shared) is type(g)
    if kind != "graph":                 # a Block and a Subgraph hand the cached structure on
        assert shared.transposed_structure() is st and len(counted) == before + 1
    # transposed() on a fresh twin runs the kernel with the values
    twin = type(g)(**{f: getattr(g, f) for f in g.__dataclass_fields__ if f != "_values"})
    t = twin.transposed()
    assert len(counted) == before + 2 and counted[-1][2] is twin.val and t is twin.transposed()
    assert type(t) is (mk.Block if kind == "block" else mk.CSRGraph)
    assert t.ptr.dtype == t.idx.dtype == torch.int32 and t.val.dtype == torch.float32
    assert torch.equal(t.ptr, want[0]) and torch.equal(t.idx, want[1])
    assert torch.equal(t.val.view(torch.int32), want[3].view(torch.int32))
    if kind == "block":
        assert t.num_src == g.num_dst and t.num_dst == g.num_src
    # after an edit of the values the cached structure is gathered, not sorted again
    g.val.mul_(2)
    t2 = g.transposed()
    assert len(counted) == before + 2 and torch.equal(t2.val, g.val[st[2]])
    COVERED.update(tr.kernels(g._num_cols(), False) | tr.kernels(g._num_cols(), True))


def test_registered_operator(gpu):
    import maxk_kernels.torch_ops  # noqa: F401
    ptr, idx, nc = tr.cases()["rect"]
    ptr_d, idx_d = dev_of(ptr, gpu), dev_of(idx, gpu)
    val_d = dev_of(tr.values(idx.size, 6), gpu)
    for v in (None, val_d):
        want = ops.csr_transpose(ptr_d, idx_d, v, nc)
        got = torch.ops.maxk.csr_transpose(ptr_d, idx_d, v, nc)
        assert len(got) == 4 and got[3].numel() == (0 if v is None else idx.size)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g.view(torch.int32), w.view(torch.int32))
        # opcheck compares its runs by value, where a NaN differs from itself: finite values
        finite = None if v is None else torch.rand(idx.size, device=gpu)
        torch.library.opcheck(torch.ops.maxk.csr_transpose.default, (ptr_d, idx_d, finite, nc))
        COVERED.update(tr.kernels(nc, v is not None))


# one backward per consumer of A^T: bit-equal between the kernel's structure and the torch path's
D, K, H = 64, 8, 4


def twin_from_torch(g):
    """A graph on g's tensors whose cached A^T comes from the torch helper."""
    twin = type(g)(**{f: getattr(g, f) for f in g.__dataclass_fields__ if f != "_values"})
    ptr_t, idx_t, order, val_t = torch_path(g)
    twin._values["transposed_structure"] = (ptr_t, idx_t, order)
    twin._values["transposed_order"] = order.to(torch.int32).contiguous()
    key = ("transposed", twin.val.data_ptr(), ops._version(twin.val))
    twin._values[key] = twin._transposed_graph(ptr_t, idx_t, val_t)
    return twin


def grads_of(consumer, g, dev):
    torch.manual_seed(31)
    nc, n, e = g._num_cols(), g.num_nodes, g.num_edges
    if consumer == "dense":
        leaves = [torch.randn(nc, D, device=dev, requires_grad=True)]
        out = mk.dense_aggregate(leaves[0], g)
    elif consumer == "gat_attention":
        leaves = [torch.randn(nc, device=dev, requires_grad=True),
                  torch.randn(n, device=dev, requires_grad=True)]
        out = mk.gat_attention(g, leaves[0], leaves[1], 0.2)
    elif consumer == "block_aggregate":
        leaves = [torch.randn(nc, D, device=dev, requires_grad=True)]
        out = mk.block_aggregate(leaves[0], g, K)
    else:
        x = torch.randn(nc, D, device=dev, requires_grad=True)
        sp_data, sp_index = mk.maxk(x, K)
        leaves = [x]
        if consumer == "heads_aggregate":
            leaves.append(torch.rand(H, e, device=dev, requires_grad=True))
            out = mk.heads_aggregate(g, leaves[1], sp_data, sp_index, D)
        else:
            out = mk.max_aggregate(g, sp_data, sp_index, D)
    out.backward(torch.randn_like(out))
    return [out.detach()] + [v.grad for v in leaves]


@pytest.mark.parametrize("consumer", ["dense", "gat_attention", "heads_aggregate", "max_aggregate",
                                      "block_aggregate"])
def test_backwards_on_the_kernels_structure_equal_the_torch_paths(gpu, counted, consumer):
    g = graphs_on(gpu)["block" if consumer == "block_aggregate" else "graph"]
    twin = twin_from_torch(g)
    before = len(counted)
    got = grads_of(consumer, g, gpu)
    assert len(counted) == before + 1, "the backward did not transpose with the kernel"
    want = grads_of(consumer, twin, gpu)
    assert len(counted) == before + 1, "the twin's cached structure was not used"
    assert len(got) == len(want) >= 2
    for a, b in zip(got, want):
        assert a is not None and a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), consumer
    COVERED.update(tr.kernels(g._num_cols(), consumer == "dense"))


# ------------------------------------------------------------------ 5. scan lengths
@pytest.mark.parametrize("n", scan.LENGTHS)
def test_out_ptr_scan_of_n_items(gpu, n):
    """out_ptr is scanned over num_cols + 1 = n items, on about 3,000 edges that name the first
    and the last column. One item means no column, which admits no edge and so no scan: that
    length is run on the tile histograms instead (one column: one tile of one digit)."""
    if n == 1:
        ptr, idx, nc = tr.random_csr(150, 1, 3000, 5)
        assert (-(-idx.size // tr.TILE)) << tr.digit_bits(nc)[0] == 1
    else:
        ptr, idx, nc = tr.plan_case(n - 1)
    run_case(ptr, idx, nc, gpu, f"out_ptr of {n} items")


def test_histogram_scan_carries_into_a_second_round(gpu):
    """257 tiles of edges under one 11-bit digit: the tile histograms are 257 scan tiles long,
    one more than a round of the scan's middle step takes."""
    nc, e = 2 ** tr.MAX_DIGIT_BITS, scan.ROUND * tr.TILE + 1
    assert tr.digit_bits(nc) == (tr.MAX_DIGIT_BITS,)
    assert scan.tiles((-(-e // tr.TILE)) << tr.MAX_DIGIT_BITS) == scan.ROUND + 1
    ptr, idx, _ = tr.random_csr(300, nc, e, 6)
    run_case(ptr, idx, nc, gpu, "257 tiles of an 11-bit digit")


# ------------------------------------------------------------------ 6. closure (keep last)
def test_every_transpose_instantiation_was_launched_by_a_passing_case(gpu):
    names = compiled()
    assert len(names) == 9 + len(tr.SCAN_KERNELS) == 12
    missing = sorted(names - COVERED)
    assert not missing, f"instantiations without a passing case: {missing}"
    assert not COVERED - names
