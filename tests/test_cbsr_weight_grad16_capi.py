"""CPU: maxk_cbsr_weight_grad_16 is declared, bound and refuses bad arguments on the host (made-up
device pointers: nothing reaches a GPU); its scratch size and tile report equal a restatement; the
Python surface refuses what has no 16-bit weight gradient; the maxk_wg16:: fixture is the library's
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_weight_grad16.txt")
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


def call(data=at(0), ds=0, index=at(1), is_=0, g=at(2), gs=0, dtype=BF16, table=at(3), ts=0,
         total=at(4), scratch=at(5), sbytes=None, n=100, d=256, k=16, m=256):
    if sbytes is None:
        sbytes = max(lib.maxk_cbsr_weight_grad_16_scratch_bytes(n, d, k, m), 0)
    return lib.maxk_cbsr_weight_grad_16(data, ds, index, is_, g, gs, dtype, table, ts, total,
                                        scratch, sbytes, n, d, k, m, None)


def restated(n, d, k, m):  # (tile report, scratch bytes) as the header words them
    dp = 64 if d <= 64 else 128 if d <= 128 else 256
    mp = 128 if m > 64 else 64
    panels = -(-m // mp)
    cap = max(256 // panels, 1)
    w = min(max(-(-n // 64), 1), cap)
    lds = 2 * (dp * (64 + 8) + 64 * (mp + 16))
    return (dp, mp, panels, 64, cap, lds), 4 * (panels * w * d * mp + w * d)


@pytest.mark.parametrize("d,m", [(1, 1), (64, 64), (65, 65), (128, 129), (129, 260), (256, 256),
                                 (256, 128 * 300)])
def test_tile_report_and_scratch_size_equal_the_restatement(d, m):
    for n in (0, 1, 64, 65, 64 * 127 + 1, 64 * 128 + 1, 232965):
        tile, scratch = restated(n, d, 1, m)
        assert ops.cbsr_weight_grad_16_tile(d, m) == tile
        assert ops.cbsr_weight_grad_16_scratch_bytes(n, d, 1, m) == scratch
    assert ops.cbsr_weight_grad_16_tile(256, 256) == (256, 128, 2, 64, 128, 55296)
    for bad in ((-1, 8, 1, 1), (1, 257, 1, 1), (1, 8, 9, 1), (1, 8, 0, 1), (1, 8, 1, 0)):
        assert ops.cbsr_weight_grad_16_scratch_bytes(*bad) == -1
    assert [lib.maxk_cbsr_weight_grad_16_tile(d, m, None, 0) for d, m in ((257, 1), (0, 1), (8, 0))] \
        == [0, 0, 0]


W = "maxk_cbsr_weight_grad_16: "
OVERLAP = "an output overlaps an input or another output"
REFUSALS = [
    (dict(dtype=0), INVALID, "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16"),
    (dict(dtype=3, n=0), INVALID, "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16"),
    (dict(n=-1), INVALID, "num_rows must be >= 0 and dim_m >= 1"),
    (dict(m=0, dtype=F16), INVALID, "num_rows must be >= 0 and dim_m >= 1"),
    (dict(d=257), UNSUPPORTED, "dim_origin above 256 is not supported (u8 selectors)"),
    (dict(k=0), INVALID, "k must be between 1 and input dimension"),
    (dict(d=64, k=65, dtype=F16), INVALID, "k must be between 1 and input dimension"),
    (dict(m=128 * 65535 + 1, n=0), UNSUPPORTED, "dim_m beyond the grid's 65535 panels is not supported"),
    (dict(ds=15), INVALID, "data_stride must be >= k (0: k)"),
    (dict(is_=15), INVALID, "index_stride must be >= k (0: k)"),
    (dict(gs=255), INVALID, "g_stride must be >= dim_m (0: dim_m)"),
    (dict(ts=255), INVALID, "grad_table_stride must be >= dim_m (0: dim_m)"),
    (dict(sbytes=lib.maxk_cbsr_weight_grad_16_scratch_bytes(100, 256, 16, 256) - 1), INVALID,
     "scratch_bytes is below maxk_cbsr_weight_grad_16_scratch_bytes"),
    (dict(scratch=at(5, 8)), INVALID, "scratch must be 16-B aligned"),
    (dict(data=None), INVALID, "null pointer"),
    (dict(index=None, dtype=F16), INVALID, "null pointer"),
    (dict(g=None), INVALID, "null pointer"),
    (dict(table=None), INVALID, "null pointer"),
    (dict(scratch=None), INVALID, "null pointer"),
    (dict(table=at(2, 2 * 100 * 256 - 1)), INVALID, OVERLAP),  # the last byte of g
    (dict(total=at(0, 16)), INVALID, OVERLAP),
    (dict(scratch=at(3, 4096)), INVALID, OVERLAP),
]


@pytest.mark.parametrize("kw,rc,msg", REFUSALS)
def test_refusals_on_the_host(kw, rc, msg):
    got = call(**kw)
    assert got == rc, (kw, got, err())
    assert err() == W + msg, err()


def test_symbols_are_bound_and_python_refuses_what_has_no_16_bit_weight_gradient():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    for name in ("maxk_cbsr_weight_grad_16", "maxk_cbsr_weight_grad_16_scratch_bytes",
                 "maxk_cbsr_weight_grad_16_tile"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(mk.cbsr_weight_grad_16) and hasattr(torch.ops.maxk, "cbsr_weight_grad_16")
    h, w = torch.zeros(4, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="weight_grad_16=True needs bfloat16 or float16"):
        mk.linear_maxk(h, w, None, 2, fused=True, weight_grad_16=True)
    for kw in (dict(), dict(sparse_linear=True, fused_linear=True)):
        with pytest.raises(ValueError, match="weight_grad_16 needs linear_dtype"):
            mk.MaxKGCNConv(8, 8, weight_grad_16=True, **kw)
    layer = mk.MaxKGCNConv(8, 8, sparse_linear=True, fused_linear=True,
                           linear_dtype=torch.bfloat16, weight_grad_16=True)
    assert layer.weight_grad_16 and not mk.MaxKGCNConv(8, 8).weight_grad_16
    data, index = torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="g must be bfloat16 or float16"):
        ops.cbsr_weight_grad_16(data, index, torch.zeros(4, 8), 8)
    with pytest.raises(RuntimeError, match="sp_data must be a CUDA tensor"):
        ops.cbsr_weight_grad_16(data, index, torch.zeros(4, 8, dtype=torch.float16), 8)


def test_fixture_equals_the_library_and_variant_check():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_wg16::") for n in names)
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_wg16::") == names and len(names) == 13
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK, "weight_grad16"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == [n for n in names if n.endswith(">")]
