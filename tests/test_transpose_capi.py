"""CPU: the CSR-transposition entry points are declared, bound and refuse bad arguments on the host
(null or made-up device pointers: nothing reaches a GPU); the digit plan and the scratch size are
the restated ones; the numpy restatement of tests/transpose.py holds the properties the rule
promises and equals tests/gat_heads.transposed on the existing graphs; CSRGraph, Block and Subgraph
on CPU tensors give the restated structure; and the maxk_tr:: fixture is the library's set, its
pass kernels the variant tables'."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gat_heads as gh
import maxk_kernels as mk
import transpose as tr
from maxk_kernels import _lib, autograd, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_transpose.txt")
CHECK = os.path.join(ROOT, "spgemm-gnn_amd", "build", "variant_check")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_csr_transpose_scratch_bytes", "maxk_csr_transpose", "maxk_transpose_digit_bits")
P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
BASE = 1 << 24
STEP = 1 << 20


def err():
    return lib.maxk_last_error().decode()


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "CSR transposition (ABI 4)" in open(HEADER).read()
    assert lib.maxk_abi_version() == 4
    for name in ("csr_transpose", "transpose_digit_bits"):
        assert name in mk.__all__ and hasattr(mk, name), name
    assert callable(ops.csr_transpose) and callable(ops.csr_transpose_scratch_bytes)


def test_header_states_the_rule():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    for phrase in ("c(e) = clamp(idx[e], 0, num_cols - 1)",
                   "the one permutation of [0, num_edges) that is ascending in (c(e), e)",
                   "out_row[j] is the row r with ptr[r] <= out_order[j] < ptr[r + 1]",
                   "the exclusive scan of the column counts",
                   "out_val[j] = val[out_order[j]], copied bit for bit",
                   "no placement depends on the returned value of an atomic"):
        assert phrase in text, phrase


def test_restated_constants_are_the_variant_headers():
    got = tr.header_constants()
    for name, want in tr.HEADER_CONSTANTS.items():
        assert got[name] == want, (name, got[name], want)
    assert tr.TILE == tr.SUB_RUN * got["kTrWaves"] and tr.SUB_RUN % tr.WAVE == 0


# ------------------------------------------------------------------ digit plan, scratch
def plan_from_library(num_cols):
    count = lib.maxk_transpose_digit_bits(num_cols, None, 0)
    buf = (ctypes.c_int32 * 4)(*([-7] * 4))
    assert lib.maxk_transpose_digit_bits(num_cols, ctypes.cast(buf, P), 4) == count
    assert all(v == -7 for v in buf[count:])
    return tuple(buf[:count])


def test_digit_plan_against_the_restatement():
    counts = set(tr.column_counts()) | {0, 232965, 2449029, 2 ** 31 - 1, 2 ** 30, 2 ** 30 + 1}
    counts |= {2 ** b + d for b in range(23, 31) for d in (-1, 0, 1)}
    seen = set()
    for nc in sorted(counts):
        widths = plan_from_library(nc)
        assert widths == tr.digit_bits(nc) == ops.transpose_digit_bits(nc), (nc, widths)
        assert sum(widths) == tr.key_bits(nc) and max(widths) <= tr.MAX_DIGIT_BITS
        assert 1 <= len(widths) <= tr.MAX_PASSES and max(widths) - min(widths) <= 1
        assert list(widths) == sorted(widths, reverse=True)
        seen.add(len(widths))
    assert seen == {1, 2, 3}
    assert plan_from_library(1) == (0,) and plan_from_library(2 ** 22) == (11, 11)
    assert plan_from_library(2 ** 22 + 1) == (8, 8, 7)
    # capacity below the count: the first widths only
    buf = (ctypes.c_int32 * 4)(*([-7] * 4))
    assert lib.maxk_transpose_digit_bits(2 ** 22 + 1, ctypes.cast(buf, P), 2) == 3
    assert list(buf) == [8, 8, -7, -7]
    # the column counts of the GPU cases end where the largest pass count is first reached
    assert tr.column_counts()[-1] == 2 ** 22 + 1 and tr.column_counts()[:3] == [1, 2, 3]


def test_scratch_size_against_the_restatement():
    for nc in (0, 1, 2, 600, 2048, 2049, 232965, 2449029, 2 ** 22 + 1):
        for e in (0, 1, tr.TILE - 1, tr.TILE, tr.TILE + 1, 17000, 114_848_857, 2 ** 31 - 1):
            for n in (1, 600):
                want = tr.scratch_bytes(n, nc, e)
                assert lib.maxk_csr_transpose_scratch_bytes(n, nc, e) == want, (n, nc, e)
                assert ops.csr_transpose_scratch_bytes(n, nc, e) == want
    for bad in ((-1, 5, 5), (5, -1, 5), (5, 5, -1), (5, 5, 2 ** 31)):
        assert lib.maxk_csr_transpose_scratch_bytes(*bad) == 0
    # two passes: the pairs and the histograms; one pass: no pairs
    assert tr.scratch_bytes(1, 5000, tr.TILE) == 8 * tr.TILE + 4 * (128 + 3)
    assert tr.scratch_bytes(1, 2048, tr.TILE) == 4 * (2048 + 2)


# ------------------------------------------------------------------ refusals
def call(ptr=P(BASE), idx=P(BASE + STEP), val=None, out_ptr=P(BASE + 2 * STEP),
         out_row=P(BASE + 3 * STEP), out_order=P(BASE + 4 * STEP), out_val=None,
         scratch=P(BASE + 6 * STEP), sb=None, n=600, nc=700, e=5000):
    sb = tr.scratch_bytes(max(n, 0), max(nc, 0), min(max(e, 0), 2 ** 31 - 1)) if sb is None else sb
    return lib.maxk_csr_transpose(ptr, idx, val, out_ptr, out_row, out_order, out_val, scratch, sb,
                                  n, nc, e, None)


VAL, OUT_VAL = P(BASE + 5 * STEP), P(BASE + 7 * STEP)
REFUSALS = [
    (dict(n=-1), "sizes"), (dict(nc=-1), "sizes"), (dict(e=-1), "sizes"),
    (dict(nc=0), "without columns"), (dict(n=0), "without rows"),
    (dict(val=VAL), "both be given or both be NULL"),
    (dict(out_val=OUT_VAL), "both be given or both be NULL"),
    (dict(sb=tr.scratch_bytes(600, 700, 5000) - 1), "scratch_bytes"), (dict(sb=0), "scratch_bytes"),
    (dict(sb=-5), "scratch_bytes"),
    (dict(ptr=None), "null pointer"), (dict(idx=None), "null pointer"),
    (dict(out_ptr=None), "null pointer"), (dict(out_row=None), "null pointer"),
    (dict(out_order=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(out_ptr=None, e=0), "null pointer"),
    (dict(out_ptr=P(BASE + 4)), "overlaps"), (dict(out_row=P(BASE + STEP + 4)), "overlaps"),
    (dict(out_order=P(BASE + 3 * STEP + 4)), "overlaps"),
    (dict(out_order=P(BASE + 2 * STEP + 4 * 700)), "overlaps"),
    (dict(scratch=P(BASE + 4 * STEP + 8)), "overlaps"),
    (dict(val=VAL, out_val=P(BASE + 5 * STEP + 4)), "overlaps"),
    (dict(val=VAL, out_val=P(BASE + 4 * STEP + 4)), "overlaps"),
    (dict(val=P(BASE + 6 * STEP), out_val=OUT_VAL), "overlaps"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS)
def test_refusals_on_the_host(kw, msg):
    got = call(**kw)
    assert got == INVALID, (kw, got, err())
    assert msg in err() and "maxk_csr_transpose: " in err(), err()


def test_too_many_edges_are_unsupported():
    got = call(e=2 ** 31, sb=1 << 40)
    assert got == UNSUPPORTED and "below 2^31" in err(), (got, err())
    assert call(e=2 ** 40, sb=1 << 50) == UNSUPPORTED


def test_ops_check_their_tensors_before_the_library():
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.csr_transpose(t, t)
    import maxk_kernels.torch_ops  # noqa: F401
    # the registered operator infers its shapes without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ptr, idx = torch.empty(11, dtype=torch.int32), torch.empty(50, dtype=torch.int32)
        out = torch.ops.maxk.csr_transpose(ptr, idx, None, 17)
        assert [tuple(o.shape) for o in out] == [(18,), (50,), (50,), (0,)]
        out = torch.ops.maxk.csr_transpose(ptr, idx, torch.empty(50), 17)
        assert [tuple(o.shape) for o in out] == [(18,), (50,), (50,), (50,)]
        assert [o.dtype for o in out] == [torch.int32] * 3 + [torch.float32]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(tr.cases()))
def test_properties_of_the_restatement(name):
    ptr, idx, nc = tr.cases()[name]
    e = idx.size
    val = tr.values(e, 1)
    out_ptr, out_row, out_order, out_val = tr.transpose_ref(ptr, idx, nc, val)
    assert all(a.dtype == np.int32 for a in (out_ptr, out_row, out_order))
    assert np.array_equal(np.sort(out_order), np.arange(e))                  # a permutation
    c = np.clip(idx.astype(np.int64), 0, max(nc - 1, 0))
    key = c[out_order] * max(e, 1) + out_order
    assert (np.diff(key) > 0).all()                                          # (c, e) ascends
    assert (np.diff(c[out_order]) >= 0).all()                                # idx[order] sorted
    assert out_ptr[0] == 0 and out_ptr[-1] == e and out_ptr.size == nc + 1
    assert np.array_equal(np.diff(out_ptr), np.bincount(c, minlength=nc)[:nc])
    assert np.array_equal(out_row, gh.rows_of(ptr)[out_order])
    assert np.array_equal(out_val.view(np.uint32), val.view(np.uint32)[out_order])
    # transposing twice returns each row's columns sorted stably
    back_ptr, back_col, back_order = tr.transpose_ref(out_ptr, out_row, ptr.size - 1)
    assert np.array_equal(back_ptr, ptr)
    rows = gh.rows_of(ptr)
    want = np.lexsort((np.arange(e), c, rows))                               # (row, c, e)
    assert np.array_equal(out_order[back_order], want) and np.array_equal(back_col, c[want])


@pytest.mark.parametrize("name", ["square", "rect", "square_t", "rect_t", "one_row", "edges_8193"])
def test_restatement_equals_the_existing_one(name):
    ptr, idx, nc = tr.cases()[name]
    for got, want in zip(tr.transpose_ref(ptr, idx, nc), gh.transposed(ptr, idx, nc)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_plan_cases_hold_their_preconditions():
    for nc in (1, 2, 3, 2049, 2 ** 12, 2 ** 22 + 1):
        ptr, idx, _ = tr.plan_case(nc)
        assert idx.min() == 0 and idx.max() == nc - 1 and 2900 <= idx.size <= 3100
        shift = 0
        for w in tr.digit_bits(nc)[:-1]:
            shift += w
            assert {(1 << shift) - 1, 1 << shift} <= set(idx.tolist())
    ptr, idx, nc = tr.cases()["stray_columns"]
    assert (idx < 0).any() and (idx >= nc).any() and idx.min() == -2 ** 31
    for t in tr.SIZES:
        assert {f"edges_{t - 1}", f"edges_{t}", f"edges_{t + 1}"} <= set(tr.cases())
    assert tr.cases()["one_column"][1].size > 3 * tr.TILE
    assert 2 * tr.TILE < tr.cases()["square"][1].size


# ------------------------------------------------------------------ CPU path of the graphs
def check_graph(g, ptr, idx, nc, val):
    want = tr.transpose_ref(ptr, idx, nc, val)
    st = g.transposed_structure()
    assert st is g.transposed_structure()
    assert [t.dtype for t in st] == [torch.int32, torch.int32, torch.int64]
    for got, w in zip(st, want):
        assert np.array_equal(got.numpy(), w)
    order = g.transposed_order()
    assert order is g.transposed_order() and order.dtype == torch.int32
    assert np.array_equal(order.numpy(), want[2])
    t = g.transposed()
    assert t is g.transposed() and type(t) is (mk.Block if isinstance(g, mk.Block) else mk.CSRGraph)
    assert np.array_equal(t.ptr.numpy(), want[0]) and np.array_equal(t.idx.numpy(), want[1])
    assert np.array_equal(t.val.numpy().view(np.uint32), want[3].view(np.uint32))
    assert np.array_equal(g.out_degrees().numpy(), np.diff(want[0]))
    assert g.out_degrees().dtype == torch.int64


@pytest.mark.parametrize("name", ["square", "rect", "no_edges"])
def test_cpu_tensors_keep_the_torch_path(name, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the kernel was called for CPU tensors")
    monkeypatch.setattr(ops, "csr_transpose", refuse)
    ptr, idx, nc = tr.cases()[name]
    val = tr.values(idx.size, 2)
    args = (torch.from_numpy(ptr.copy()), torch.from_numpy(idx.copy()),
            torch.from_numpy(val.copy()))
    if nc == ptr.size - 1:
        check_graph(mk.CSRGraph(*args), ptr, idx, nc, val)
        check_graph(mk.Subgraph(*args, node_ids=torch.arange(nc, dtype=torch.int32),
                                eids=torch.arange(idx.size, dtype=torch.int32),
                                parent_num_nodes=nc), ptr, idx, nc, val)
    block = mk.Block(*args, num_src=nc)
    check_graph(block, ptr, idx, nc, val)
    assert block.transposed().num_src == ptr.size - 1
    # a fresh graph: transposed() first, then the structure
    fresh = mk.Block(*args, num_src=nc)
    t = fresh.transposed()
    assert np.array_equal(t.idx.numpy(), tr.transpose_ref(ptr, idx, nc)[1])
    shared = block.with_values("mean")
    assert shared.transposed_structure() is block.transposed_structure()
    # the private helper itself
    ptr_t, rows, order = autograd._torch_transpose(args[0], args[1], nc)
    want = tr.transpose_ref(ptr, idx, nc)
    assert ptr_t.dtype == rows.dtype == order.dtype == torch.int64
    assert np.array_equal(ptr_t.numpy(), want[0]) and np.array_equal(order.numpy(), want[2])
    assert np.array_equal(rows[order].numpy(), want[1])


# ------------------------------------------------------------------ fixtures, tables
def test_restated_names_cover_the_fixture():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_tr::") for n in names)
    own = set(tr.COMMON_KERNELS) - set(tr.SCAN_KERNELS)
    assert set(names) == tr.pass_kernel_names() | own and len(names) == 9
    assert all(n.startswith("maxk_scan::") for n in tr.SCAN_KERNELS)
    for nc in (1, 5000, 2 ** 22 + 1):
        for v in (False, True):
            assert tr.kernels(nc, v) <= set(names) | set(tr.SCAN_KERNELS)


def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_tr::") == kernel_list.read_list(FIXTURE)
    assert kernel_list.main([_lib.LIB_PATH, "--namespace", "maxk_tr::", "--diff", FIXTURE]) == 0


def test_variant_check_names_the_fixtures_pass_kernels():
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK, "transpose"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stderr
    want = [n for n in kernel_list.read_list(FIXTURE) if n not in tr.COMMON_KERNELS]
    assert run.stdout.splitlines() == want and set(want) == tr.pass_kernel_names()
