"""CPU: the CBSR-times-table entry points are declared, bound and refuse bad arguments on the host
(made-up device pointers: nothing reaches a GPU); scratch sizes and panel plan are the restated
ones; the float64 restatements of tests/cbsr_linear.py are adjoint to each other; the maxk_lin::
fixture is the library's set, its panel kernels the variant tables'."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cbsr_linear as cl
import maxk_kernels as mk
from maxk_kernels import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_linear.txt")
CHECK = os.path.join(ROOT, "spgemm-gnn_amd", "build", "variant_check")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_cbsr_matmul", "maxk_cbsr_sampled_matmul", "maxk_cbsr_weight_grad",
       "maxk_cbsr_linear_scratch_bytes", "maxk_cbsr_linear_panel")
P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
STEP = 1 << 24


def at(i, off=0):
    return P((1 << 30) + i * STEP + off)


def err():
    return lib.maxk_last_error().decode()


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "MaxK linear layers (ABI 4)" in open(HEADER).read() and lib.maxk_abi_version() == 4
    for name in ("cbsr_matmul", "cbsr_sampled_matmul", "cbsr_weight_grad", "cbsr_linear",
                 "linear_maxk"):
        assert name in mk.__all__ and hasattr(mk, name), name
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.cbsr_matmul(torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.uint8), torch.zeros(8, 3))
    with pytest.raises(ValueError, match="ref_compat"):
        mk.linear_maxk(torch.zeros(4, 8), torch.zeros(8, 8), None, 2, mode="ref_compat")


# ------------------------------------------------------------------ refusals
def matmul(data=at(0), ds=0, sel=at(1), is_=0, T=at(2), ts=0, bias=at(3), out=at(4), os_=0,
           n=100, D=256, k=16, m=256, **_):
    return lib.maxk_cbsr_matmul(data, ds, sel, is_, T, ts, bias, out, os_, n, D, k, m, None)


def sampled_matmul(g=at(0), gs=0, sel=at(1), is_=0, T=at(2), ts=0, out=at(4), os_=0, scratch=at(5),
            sb=None, n=100, D=256, k=16, m=256, **_):
    sb = max(cl.scratch_bytes(cl.SAMPLED, max(n, 0), D, k, m), 0) if sb is None else sb
    return lib.maxk_cbsr_sampled_matmul(g, gs, sel, is_, T, ts, out, os_, scratch, sb, n, D, k, m,
                                        None)


def weight_grad(data=at(0), ds=0, sel=at(1), is_=0, g=at(2), gs=0, out=at(4), os_=0, dsum=at(3),
                scratch=at(5), sb=None, n=100, D=256, k=16, m=256, **_):
    sb = max(cl.scratch_bytes(cl.WEIGHT_GRAD, max(n, 0), D, k, m), 0) if sb is None else sb
    return lib.maxk_cbsr_weight_grad(data, ds, sel, is_, g, gs, out, os_, dsum, scratch, sb, n, D,
                                     k, m, None)


ALL = (matmul, sampled_matmul, weight_grad)
REFUSALS = [
    (ALL, dict(n=-1), INVALID, "num_rows must be >= 0 and dim_m >= 1"),
    (ALL, dict(m=0), INVALID, "num_rows must be >= 0 and dim_m >= 1"),
    (ALL, dict(D=257), UNSUPPORTED, "dim_origin above 256 is not supported"),
    (ALL, dict(k=0), INVALID, "k must be between 1 and input dimension"),
    (ALL, dict(D=64, k=65), INVALID, "k must be between 1 and input dimension"),
    (ALL, dict(m=65535 * 128 + 1, sb=1 << 50), UNSUPPORTED, "beyond the grid's 65535 panels"),
    (ALL, dict(is_=15), INVALID, "index_stride must be >= k"),
    ((matmul, weight_grad), dict(ds=15), INVALID, "data_stride must be >= k"),
    ((matmul, sampled_matmul), dict(ts=255), INVALID, "table_stride must be >= dim_m"),
    ((sampled_matmul, weight_grad), dict(gs=255), INVALID, "g_stride must be >= dim_m"),
    ((matmul,), dict(os_=255), INVALID, "out_stride must be >= dim_m"),
    ((sampled_matmul,), dict(os_=15), INVALID, "out_stride must be >= k"),
    ((weight_grad,), dict(os_=255), INVALID, "grad_table_stride must be >= dim_m"),
    ((sampled_matmul, weight_grad), dict(sb=1000), INVALID, "scratch_bytes is below"),
    ((sampled_matmul, weight_grad), dict(scratch=at(5, 4)), INVALID, "scratch must be 16-B aligned"),
    ((sampled_matmul, weight_grad), dict(scratch=None), INVALID, "null pointer"),
    (ALL, dict(sel=None), INVALID, "null pointer"),
    (ALL, dict(out=None), INVALID, "null pointer"),
    ((matmul, sampled_matmul), dict(T=None), INVALID, "null pointer"),
    ((matmul, weight_grad), dict(data=None), INVALID, "null pointer"),
    ((sampled_matmul, weight_grad), dict(g=None), INVALID, "null pointer"),
    (ALL, dict(out=at(1, 16)), INVALID, "overlaps"),
    ((matmul,), dict(out=at(3, 4)), INVALID, "overlaps"),
    ((sampled_matmul, weight_grad), dict(scratch=at(4, 16)), INVALID, "overlaps"),
    ((weight_grad,), dict(dsum=at(4, 64)), INVALID, "overlaps"),
    # a strided out reaches from its base into the next array
    ((matmul,), dict(out=at(1, 4096), os_=STEP // 4 // 50), INVALID, "overlaps"),
]


@pytest.mark.parametrize("calls,kw,rc,msg", REFUSALS)
def test_refusals_on_the_host(calls, kw, rc, msg):
    for call in calls:
        got = call(**kw)
        assert got == rc, (call.__name__, kw, got, err())
        assert msg in err() and err().startswith(f"maxk_cbsr_{call.__name__}: "), err()


def test_optional_arrays_and_empty_inputs():
    # nothing to do without rows, whatever the pointers; the weight gradient still writes zeros
    assert matmul(n=0, data=None, sel=None, out=None) == 0
    assert sampled_matmul(n=0, g=None, sel=None, out=None, scratch=None) == 0
    assert weight_grad(n=0, out=None) == INVALID and "null pointer" in err()
    # bias and grad_sum are optional: the refusal that follows is not about them
    assert matmul(bias=None, out=at(2, 16)) == INVALID and "overlaps" in err()
    assert weight_grad(dsum=None, out=at(2, 16)) == INVALID and "overlaps" in err()


# ------------------------------------------------------------------ scratch, panels
def test_scratch_bytes_and_panel_against_the_restatement():
    for d in (1, 16, 100, 256):
        for m in (1, 4, 63, 64, 65, 127, 128, 129, 256, 260, 644, 32768):
            buf = (ctypes.c_int32 * 3)(-7, -7, -7)
            assert lib.maxk_cbsr_linear_panel(d, m, ctypes.cast(buf, P), 3) == 2
            assert tuple(buf) == cl.panel(d, m) + (-7,) and ops.cbsr_linear_panel(d, m) == cl.panel(d, m)
            for n in (0, 1, 16, 17, 1000, 4096, 4097, 232965, 2449029):
                for op in (0, 1, 2, 3, -1):
                    want = cl.scratch_bytes(op, n, d, min(d, 16), m)
                    assert lib.maxk_cbsr_linear_scratch_bytes(op, n, d, min(d, 16), m) == want
    assert cl.scratch_bytes(cl.WEIGHT_GRAD, 232965, 256, 16, 256) == 4 * 256 * (256 * 128 + 128)
    for bad in ((0, -1, 8, 1, 1), (0, 1, 8, 9, 1), (0, 1, 257, 1, 1), (0, 1, 8, 0, 1),
                (0, 1, 8, 1, 0)):
        assert lib.maxk_cbsr_linear_scratch_bytes(*bad) == -1 == cl.scratch_bytes(*bad)
    assert lib.maxk_cbsr_linear_panel(257, 4, None, 0) == 0 == lib.maxk_cbsr_linear_panel(8, 0, None, 0)


# ------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("n,d,k,m", cl.CASES[:8])
@pytest.mark.parametrize("repeat", [False, True])
def test_restatements_are_adjoint(n, d, k, m, repeat):
    """<out_A, g> = <v, out_B> = <T, dT>, and dsum is dT for a g of ones."""
    v, s, T, g, _ = cl.inputs(n, d, k, m, 3, exact=False, repeat=repeat)
    out_a, mag_a = cl.matmul64(v, s, T)
    out_b = cl.sampled64(g, s, T)[0]
    dT, dsum, _, mag_sum, count = cl.weight_grad64(v, s, g, d)
    a, b, c = (out_a * g).sum(), (v * out_b).sum(), (T * dT).sum()
    scale = (mag_a * np.abs(g)).sum()
    assert abs(a - b) <= 1e-12 * scale and abs(a - c) <= 1e-12 * scale
    ones = cl.weight_grad64(v, s, np.ones((n, 1), np.float32), d)[0][:, 0]
    assert np.allclose(ones, dsum, rtol=0, atol=1e-12 * mag_sum.max())
    assert count.sum() == n * k and ((count == 0) <= (mag_sum == 0)).all()
    assert not (repeat and k > 1) or (s[:, 1] == s[:, 0]).all()


# ------------------------------------------------------------------ fixtures, tables
def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_lin::") for n in names)
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_lin::") == names and len(names) == 8
    assert kernel_list.main([_lib.LIB_PATH, "--namespace", "maxk_lin::", "--diff", FIXTURE]) == 0
    assert set().union(*(cl.kernels(d, m) for _, d, _, m in cl.CASES)) == set(names)


def test_variant_check_names_the_fixtures_panel_kernels():
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK, "linear"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stderr
    want = [n for n in kernel_list.read_list(FIXTURE) if n.endswith(">")]
    assert run.stdout.splitlines() == want and len(want) == 6
