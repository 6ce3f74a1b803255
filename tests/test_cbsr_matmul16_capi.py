"""CPU: maxk_cbsr_matmul_16 is declared, bound and refuses bad arguments on the host (made-up
device pointers: nothing reaches a GPU); its tile report equals a restatement of the header; the
Python surface refuses what has no 16-bit input gradient; the maxk_mm16:: fixture is the library's
set and variant_check's names."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_matmul16.txt")
CHECK = os.path.join(ROOT, "spgemm-gnn_amd", "build", "variant_check")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
STEP = 1 << 26
BF16, F16 = 1, 2


def at(i, off=0):
    return P((1 << 30) + i * STEP + off)


def err():
    return lib.maxk_last_error().decode()


def call(data=at(0), ds=0, index=at(1), is_=0, table=at(2), ts=0, dtype=BF16, out=at(3), os_=0,
         out_dtype=0, n=100, d=256, k=16, m=256):
    return lib.maxk_cbsr_matmul_16(data, ds, index, is_, table, ts, dtype, out, os_, out_dtype,
                                   n, d, k, m, None)


def restated(d, m):  # the tile report as the header words it
    dp = 64 if d <= 64 else 128 if d <= 128 else 256
    mp = 128 if m > 64 else 64
    panels = -(-m // mp)
    return dp, mp, panels, 128, max(256 // panels, 1), 2 * (dp * (mp + 16) + 128 * (dp + 8))


@pytest.mark.parametrize("d,m", [(1, 1), (64, 64), (65, 65), (128, 129), (129, 260), (256, 256),
                                 (256, 128 * 300)])
def test_tile_report_equals_the_restatement(d, m):
    assert ops.cbsr_matmul_16_tile(d, m) == restated(d, m)
    assert ops.cbsr_matmul_16_tile(256, 256) == (256, 128, 2, 128, 128, 141312)
    assert ops.cbsr_matmul_16_tile(d, m)[5] <= 160 * 1024
    assert [lib.maxk_cbsr_matmul_16_tile(d, m, None, 0) for d, m in ((257, 1), (0, 1), (8, 0))] \
        == [0, 0, 0]


W = "maxk_cbsr_matmul_16: "
OVERLAP = "an output overlaps an input or another output"
REFUSALS = [
    (dict(dtype=0), INVALID, "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16"),
    (dict(dtype=3, n=0), INVALID, "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16"),
    (dict(out_dtype=F16), INVALID, "out_dtype must be 0 (f32) or dtype"),
    (dict(dtype=F16, out_dtype=3), INVALID, "out_dtype must be 0 (f32) or dtype"),
    (dict(n=-1), INVALID, "num_rows must be >= 0 and dim_m >= 1"),
    (dict(m=0, dtype=F16), INVALID, "num_rows must be >= 0 and dim_m >= 1"),
    (dict(d=257), UNSUPPORTED, "dim_origin above 256 is not supported (u8 selectors)"),
    (dict(k=0), INVALID, "k must be between 1 and input dimension"),
    (dict(d=64, k=65, dtype=F16), INVALID, "k must be between 1 and input dimension"),
    (dict(m=128 * 65535 + 1, n=0), UNSUPPORTED, "dim_m beyond the grid's 65535 panels is not supported"),
    (dict(ds=15), INVALID, "data_stride must be >= k (0: k)"),
    (dict(is_=15), INVALID, "index_stride must be >= k (0: k)"),
    (dict(ts=255), INVALID, "table_stride must be >= dim_m (0: dim_m)"),
    (dict(os_=255, out_dtype=BF16), INVALID, "out_stride must be >= dim_m (0: dim_m)"),
    (dict(data=None), INVALID, "null pointer"),
    (dict(index=None, dtype=F16), INVALID, "null pointer"),
    (dict(table=None), INVALID, "null pointer"),
    (dict(out=None), INVALID, "null pointer"),
    (dict(out=at(2, 2 * 256 * 256 - 1)), INVALID, OVERLAP),  # the last byte of the table
    (dict(out=at(0, 16), out_dtype=BF16), INVALID, OVERLAP),
    (dict(out=at(1, -2 * 100 * 256 + 1), out_dtype=BF16), INVALID, OVERLAP),  # its last byte on index
]


@pytest.mark.parametrize("kw,rc,msg", REFUSALS)
def test_refusals_on_the_host(kw, rc, msg):
    got = call(**kw)
    assert got == rc, (kw, got, err())
    assert err() == W + msg, err()


def test_no_rows_is_ok_before_any_device_call():
    assert call(n=0) == 0 and call(n=0, out=None, dtype=F16, out_dtype=F16) == 0


def test_symbols_are_bound_and_python_refuses_what_has_no_16_bit_input_gradient():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    for name in ("maxk_cbsr_matmul_16", "maxk_cbsr_matmul_16_tile"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(mk.cbsr_matmul_16) and "cbsr_matmul_16" in mk.__all__
    assert hasattr(torch.ops.maxk, "cbsr_matmul_16")
    h, w = torch.zeros(4, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="input_grad_16=True needs bfloat16 or float16"):
        mk.linear_maxk(h, w, None, 2, fused=True, input_grad_16=True)
    for kw in (dict(), dict(sparse_linear=True, fused_linear=True)):
        with pytest.raises(ValueError, match="input_grad_16 needs linear_dtype"):
            mk.MaxKGCNConv(8, 8, input_grad_16=True, **kw)
    layer = mk.MaxKGCNConv(8, 8, sparse_linear=True, fused_linear=True,
                           linear_dtype=torch.bfloat16, input_grad_16=True)
    assert layer.input_grad_16 and not mk.MaxKGCNConv(8, 8).input_grad_16
    data, index = torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="table must be bfloat16 or float16"):
        ops.cbsr_matmul_16(data, index, torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="sp_data must be a CUDA tensor"):
        ops.cbsr_matmul_16(data, index, torch.zeros(8, 8, dtype=torch.float16))


def test_fixture_equals_the_library_and_variant_check():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_mm16::") for n in names)
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_mm16::") == names and len(names) == 12
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK, "matmul16"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == names
