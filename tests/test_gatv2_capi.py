"""CPU: the MaxK GATv2 entry points are declared, bound, exported and refuse bad arguments on the
host (null device pointers throughout: nothing reaches a GPU); the restatements of tests/gatv2.py
at k = D are dglnn.GATv2Conv's dense formula; and the maxk_v2:: fixture is the library's set."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import gat_heads as gh
import gatv2 as gv
import maxk_kernels as mk
from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_gatv2.txt")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_gatv2_score_forward", "maxk_edge_softmax_forward_heads",
       "maxk_edge_softmax_backward_heads", "maxk_gatv2_score_backward_rows",
       "maxk_gatv2_score_backward_cols", "maxk_gatv2_scratch_bytes", "maxk_gatv2_row_limits")
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    for name in ("edge_softmax_heads", "gatv2_attention", "MaxKGATv2Conv"):
        assert name in mk.__all__ and hasattr(mk, name), name
    assert mk.ops.gatv2_row_limits() == gh.LIMITS
    assert lib.maxk_gatv2_scratch_bytes(600, 256) == 4 * 256 * 38
    assert lib.maxk_gatv2_scratch_bytes(1 << 20, 64) == 4 * 64 * gv.MAX_PARTIALS
    assert lib.maxk_gatv2_scratch_bytes(-1, 64) == -1 == lib.maxk_gatv2_scratch_bytes(10, 257)


def fwd(H=8, n=10, nc=10, e=100, D=256, k=16, **_):
    return lib.maxk_gatv2_score_forward(None, None, None, 0, None, 0, None, 0, None, 0.2, None,
                                        H, n, nc, e, D, k, None)


def rows(H=8, n=10, nc=10, e=100, D=256, k=16, sbytes=1 << 20):
    return lib.maxk_gatv2_score_backward_rows(None, None, None, 0, None, 0, None, 0, None, 0.2,
                                              None, None, None, None, sbytes, H, n, nc, e, D, k,
                                              None)


def cols(H=8, n=10, nc=10, e=100, D=256, k=16, **_):
    return lib.maxk_gatv2_score_backward_cols(None, None, None, None, 0, None, 0, None, 0, None,
                                              0.2, None, None, H, n, nc, e, D, k, None)


@pytest.mark.parametrize("call", [fwd, rows, cols])
@pytest.mark.parametrize("kw,rc,msg", [
    (dict(), INVALID, "null pointer"),
    (dict(H=3), INVALID, "num_heads must be >= 1 and divide"),       # 3 does not divide 256
    (dict(H=32), UNSUPPORTED, "above 16"),
    (dict(D=66, H=2), UNSUPPORTED, "multiple of 4"),
    (dict(D=64, k=65), INVALID, "k must be between 1 and input dimension"),
])
def test_refusals_on_the_host(call, kw, rc, msg):
    assert call(**kw) == rc, (kw, lib.maxk_last_error().decode())
    assert msg in lib.maxk_last_error().decode()


def test_a_short_scratch_is_refused():
    assert rows(sbytes=4 * 256 - 1) == INVALID
    assert "scratch_bytes" in lib.maxk_last_error().decode()


def test_softmax_heads_refusals_on_the_host():
    f, b = lib.maxk_edge_softmax_forward_heads, lib.maxk_edge_softmax_backward_heads
    for H, rc, msg in ((4, INVALID, "null pointer"), (0, INVALID, "num_heads must be >= 1"),
                       (65536, INVALID, "beyond")):
        assert f(None, None, None, H, 10, 100, None) == rc
        assert msg in lib.maxk_last_error().decode()
        assert b(None, None, None, None, H, 10, 100, None) == rc
        assert msg in lib.maxk_last_error().decode()
    assert f(None, None, None, 4, 10, 0, None) == 0 == b(None, None, None, None, 4, 0, 0, None)


def test_restatement_at_full_k_is_the_dense_formula():
    """With every feature kept, Delta differs from GATv2's score by a per-(row, head) constant,
    and the model of the restatement is the dense layer."""
    ptr, idx = gh.small_graph(40)
    D, H = 32, 4
    data, _, fd, attn, _ = gv.inputs(40, 40, idx.size, D, H, D, seed=5)
    sel = np.broadcast_to(np.arange(D, dtype=np.uint8), (40, D))
    delta, _, m = gv.score64(ptr, idx, data, sel, fd, attn)
    r = gh.rows_of(ptr)
    a = attn.reshape(-1).astype(np.float64)
    dense = (a * gv.lrelu(data[idx].astype(np.float64) + fd[r])).reshape(-1, H, D // H).sum(-1)
    const = (a * gv.lrelu(fd.astype(np.float64))).reshape(-1, H, D // H).sum(-1)
    assert np.allclose(delta.T + const[r], dense, rtol=1e-12, atol=1e-12) and m.max() == D // H
    rng = torch.Generator().manual_seed(3)
    p = {n: torch.randn(s, generator=rng, dtype=torch.float64)
         for n, s in (("w_src", (D, 12)), ("b_src", (D,)), ("w_dst", (D, 12)), ("b_dst", (D,)),
                      ("attn", (H, D // H)))}
    feat = torch.randn(40, 12, generator=rng, dtype=torch.float64)
    full = torch.arange(D).expand(40, D)
    assert torch.allclose(gv.model64(ptr, idx, feat, p, H, full), gv.model64(ptr, idx, feat, p, H),
                          rtol=1e-10, atol=1e-12)


def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    names = kernel_list.read_list(FIXTURE)
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_v2::") == names and len(names) == 18
