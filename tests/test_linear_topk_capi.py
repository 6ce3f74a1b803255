"""CPU: maxk_linear_topk is declared, bound and refuses bad arguments on the host (made-up device
pointers: nothing reaches a GPU); num_rows == 0 is a no-op; the maxk_lt:: fixture is the library's
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_linear_topk.txt")
CHECK = os.path.join(ROOT, "spgemm-gnn_amd", "build", "variant_check")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
STEP = 1 << 24


def at(i, off=0):
    return P((1 << 30) + i * STEP + off)


def err():
    return lib.maxk_last_error().decode()


def call(h=at(0), hs=0, w=at(1), ws=0, bias=at(2), n=100, d_in=256, d=256, k=16, data=at(3), ds=0,
         index=at(4), is_=0, dense=at(5), dstride=0):
    return lib.maxk_linear_topk(h, hs, w, ws, bias, n, d_in, d, k, data, ds, index, is_, dense,
                                dstride, None)


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("maxk_linear_topk", "maxk_linear_topk_tile"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "linear_topk" in mk.__all__ and hasattr(torch.ops.maxk, "linear_topk")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.linear_topk(torch.zeros(4, 8), torch.zeros(8, 8), None, 2)
    assert ops.linear_topk_tile(256) == (64, 256, 32, 46080)
    assert [ops.linear_topk_tile(d)[1] for d in (1, 64, 65, 128, 129)] == [64, 64, 128, 128, 256]
    assert lib.maxk_linear_topk_tile(257, None, 0) == 0 == lib.maxk_linear_topk_tile(0, None, 0)


REFUSALS = [
    (dict(n=-1), INVALID, "num_rows must be >= 0 and dim_in >= 1"),
    (dict(d_in=0), INVALID, "num_rows must be >= 0 and dim_in >= 1"),
    (dict(d=257), UNSUPPORTED, "dim_origin above 256 is not supported"),
    (dict(k=0), INVALID, "k must be between 1 and input dimension"),
    (dict(d=64, k=65), INVALID, "k must be between 1 and input dimension"),
    (dict(d=0, k=1), INVALID, "k must be between 1 and input dimension"),
    (dict(hs=255), INVALID, "h_stride must be >= dim_in"),
    (dict(ws=255), INVALID, "w_stride must be >= dim_in"),
    (dict(ds=15), INVALID, "data_stride must be >= k"),
    (dict(is_=15), INVALID, "index_stride must be >= k"),
    (dict(dstride=255), INVALID, "dense_stride must be >= dim_origin"),
    (dict(h=None), INVALID, "null pointer"),
    (dict(w=None), INVALID, "null pointer"),
    (dict(data=None), INVALID, "null pointer"),
    (dict(index=None), INVALID, "null pointer"),
    (dict(dense=at(0, 64)), INVALID, "overlaps"),          # dense over h
    (dict(data=at(1, 16)), INVALID, "overlaps"),           # a table over the weight
    (dict(index=at(2, 4)), INVALID, "overlaps"),           # a table over the bias
    (dict(dense=at(2, 4096), dstride=STEP // 4 // 50), INVALID, "overlaps"),  # strided into a table
]


@pytest.mark.parametrize("kw,rc,msg", REFUSALS)
def test_refusals_on_the_host(kw, rc, msg):
    got = call(**kw)
    assert got == rc, (kw, got, err())
    assert msg in err() and err().startswith("maxk_linear_topk: "), err()


def test_optional_arrays_and_empty_input():
    assert call(n=0, h=None, w=None, bias=None, data=None, index=None, dense=None) == 0
    assert call(n=0, d=257) == UNSUPPORTED and call(n=0, ds=3) == INVALID  # sizes still checked
    # bias and dense are optional: the refusal that follows is not about them
    assert call(bias=None, dense=None, data=at(0, 16)) == INVALID and "overlaps" in err()


def test_fixture_equals_the_library_and_variant_check():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_lt::") for n in names)
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_lt::") == names and len(names) == 6
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK, "linear_topk"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == names
