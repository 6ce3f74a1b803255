"""CPU: maxk_linear_topk_16 is declared, bound and refuses bad arguments on the host (made-up device
pointers: nothing reaches a GPU); num_rows == 0 is a no-op; the Python surface refuses what has no
16-bit kernel; the maxk_lt16:: fixture is the library's set and variant_check's names."""
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_linear_topk16.txt")
CHECK = os.path.join(ROOT, "spgemm-gnn_amd", "build", "variant_check")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
STEP = 1 << 24
BF16, F16 = 1, 2


def at(i, off=0):
    return P((1 << 30) + i * STEP + off)


def err():
    return lib.maxk_last_error().decode()


def call(h=at(0), hs=0, w=at(1), ws=0, bias=at(2), dtype=BF16, n=100, d_in=256, d=256, k=16,
         data=at(3), ds=0, index=at(4), is_=0, dense=at(5), dstride=0):
    return lib.maxk_linear_topk_16(h, hs, w, ws, bias, dtype, n, d_in, d, k, data, ds, index, is_,
                                   dense, dstride, None)


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("maxk_linear_topk_16", "maxk_linear_topk_16_tile"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    codes = dict(re.findall(r"\b(MAXK_DTYPE_\w+)\s*=\s*(\d+)", text))
    assert codes == {"MAXK_DTYPE_BF16": str(BF16), "MAXK_DTYPE_F16": str(F16)}
    assert ops.LINEAR_TOPK_DTYPES == {torch.bfloat16: BF16, torch.float16: F16}
    for dt in ops.LINEAR_TOPK_DTYPES:
        assert ops.linear_topk_tile(256, dt) == (128, 256, 64, 55296)
    assert [ops.linear_topk_tile(d, torch.float16)[1] for d in (1, 64, 65, 129)] == [64, 64, 128, 256]
    assert ops.linear_topk_tile(256) == ops.linear_topk_tile(256, torch.float32)
    assert lib.maxk_linear_topk_16_tile(257, None, 0) == 0 == lib.maxk_linear_topk_16_tile(0, None, 0)


REFUSALS = [
    (dict(dtype=0), INVALID, "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16"),
    (dict(dtype=3, n=0), INVALID, "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16"),
    (dict(n=-1), INVALID, "num_rows must be >= 0 and dim_in >= 1"),
    (dict(d_in=0, dtype=F16), INVALID, "num_rows must be >= 0 and dim_in >= 1"),
    (dict(d=257), UNSUPPORTED, "dim_origin above 256 is not supported"),
    (dict(k=0), INVALID, "k must be between 1 and input dimension"),
    (dict(d=64, k=65, dtype=F16), INVALID, "k must be between 1 and input dimension"),
    (dict(d=0, k=1), INVALID, "k must be between 1 and input dimension"),
    (dict(hs=255), INVALID, "h_stride must be >= dim_in"),
    (dict(ws=255), INVALID, "w_stride must be >= dim_in"),
    (dict(ds=15), INVALID, "data_stride must be >= k"),
    (dict(is_=15), INVALID, "index_stride must be >= k"),
    (dict(dstride=255), INVALID, "dense_stride must be >= dim_origin"),
    (dict(h=None), INVALID, "null pointer"),
    (dict(w=None, dtype=F16), INVALID, "null pointer"),
    (dict(data=None), INVALID, "null pointer"),
    (dict(index=None), INVALID, "null pointer"),
    (dict(dense=at(0, 64)), INVALID, "overlaps"),          # dense over h
    (dict(data=at(1, 16)), INVALID, "overlaps"),           # a table over the weight
    (dict(index=at(2, 4)), INVALID, "overlaps"),           # a table over the bias
    (dict(dense=at(2, 4096), dstride=STEP // 4 // 50), INVALID, "overlaps"),  # strided into a table
    (dict(data=at(0, 2 * 100 * 256 - 1)), INVALID, "overlaps"),  # the last byte of h
]


@pytest.mark.parametrize("kw,rc,msg", REFUSALS)
def test_refusals_on_the_host(kw, rc, msg):
    got = call(**kw)
    assert got == rc, (kw, got, err())
    assert msg in err() and err().startswith("maxk_linear_topk_16: "), err()


def test_optional_arrays_and_empty_input():
    for dt in (BF16, F16):
        assert call(n=0, dtype=dt, h=None, w=None, bias=None, data=None, index=None,
                    dense=None) == 0
    assert call(n=0, d=257) == UNSUPPORTED and call(n=0, ds=3) == INVALID == call(n=0, dtype=7)
    # bias and dense are optional: the refusal that follows is not about them
    assert call(bias=None, dense=None, data=at(0, 16)) == INVALID and "overlaps" in err()


def test_python_surface_refuses_what_has_no_16_bit_kernel():
    h, w = torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.linear_topk(h, w, None, 2)
    with pytest.raises(ValueError, match="fused=True"):
        mk.linear_maxk(h, w, None, 2, fused=False)
    with pytest.raises(ValueError, match="fused=True"):
        mk.linear_maxk(h.half(), w.half(), None, 2)
    for kw in (dict(), dict(sparse_linear=True), dict(fused_linear=True)):
        with pytest.raises(ValueError, match="fused_linear"):
            mk.MaxKGCNConv(8, 8, linear_dtype=torch.bfloat16, **kw)
    layer = mk.MaxKGCNConv(8, 8, sparse_linear=True, fused_linear=True, linear_dtype=torch.float16)
    assert layer.linear_dtype == torch.float16 and layer.weight.dtype == torch.float32
    for a, b, msg in ((torch.bfloat16, torch.float32, "one dtype"),
                      (torch.float16, torch.bfloat16, "one dtype"),
                      (torch.float64, torch.float64, "float32, bfloat16 or")):
        with pytest.raises(RuntimeError, match=msg):
            ops.linear_topk(torch.zeros(4, 8, dtype=a), torch.zeros(8, 8, dtype=b), None, 2)


def test_fixture_equals_the_library_and_variant_check():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_lt16::") for n in names)
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_lt16::") == names and len(names) == 12
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK, "linear_topk16"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == names
