"""CPU: the fused-dropout entry points (maxk_topk_cbsr_dropout, maxk_scatter_backward_dropout)
are declared, bound, and refuse bad arguments on the host before any device call; and the
numpy restatement of the mask of include/maxk_hip.h ("Dropout mask"), which the GPU tests of
test_gpu_dropout.py compare the kernels against bit for bit, has the statistics of a dropout
mask."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -2
GOLD = np.uint32(0x9E3779B1)


# ------------------------------------------------------------------ the mask, in numpy
def fmix32(x):
    """murmur3 finaliser on uint32 arrays (array arithmetic wraps)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def drop_threshold(p) -> int:
    """T = min(2^32 - 1, (uint64)((double)(float)p * 2^32))."""
    return min(2 ** 32 - 1, int(float(np.float32(p)) * 4294967296.0))


def drop_scale(p) -> np.float32:
    pf = np.float32(p)
    return np.float32(0.0) if pf >= 1 else np.float32(1.0) / (np.float32(1.0) - pf)


def keep_mask(p, seed, rows, feats):
    """keep[r, f] for global rows ``rows`` (any int array, low 32 bits used) and feature
    indices ``feats``, broadcast against each other."""
    seed = int(seed) % 2 ** 64
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    r = (np.asarray(rows, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    f = np.asarray(feats, dtype=np.int64).astype(np.uint32)
    a = fmix32(r ^ lo)
    b = fmix32(r * GOLD + hi)
    u = fmix32(fmix32(a + GOLD * (f + np.uint32(1))) ^ b)
    if np.float32(p) >= 1:
        return np.zeros(u.shape, bool)
    return u >= np.uint32(drop_threshold(p))


def dropped_table(values, index, p, seed, row_offset=0):
    """A [n, k] f32 table after dropout at the features ``index`` [n, k]: kept entries
    fl32(x * scale), dropped entries +0.0f (also for Inf / NaN)."""
    values = np.asarray(values, dtype=np.float32)
    rows = row_offset + np.arange(values.shape[0], dtype=np.int64)[:, None]
    keep = keep_mask(p, seed, rows, index)
    with np.errstate(all="ignore"):
        scaled = (values * drop_scale(p)).astype(np.float32)
    return np.where(keep, scaled, np.float32(0.0)).astype(np.float32)


def test_threshold_and_scale_pins():
    assert drop_threshold(0.0) == 0
    assert drop_threshold(0.5) == 2147483648
    assert drop_threshold(0.999999) == 4294962944
    assert drop_threshold(1.0) == 2 ** 32 - 1
    assert drop_scale(0.5) == np.float32(2.0) and drop_scale(1.0) == 0.0
    assert drop_scale(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    # one pinned draw: fmix32 of 1 and of 0
    assert int(fmix32(np.uint32(1))) == 0x514E28B7 and int(fmix32(np.uint32(0))) == 0


SEEDS = [0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1]


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", SEEDS)
def test_keep_fraction_within_4_sigma(seed, p):
    rows = np.arange(20000)[:, None]
    feats = np.arange(256)[None, :]
    keep = keep_mask(p, seed, rows, feats)
    n = keep.size
    pf = float(np.float32(p))
    sigma = math.sqrt(pf * (1 - pf) / n)
    dev = abs(keep.mean() - (1 - pf)) / sigma
    print(f"seed {seed:#x} p {p}: keep {keep.mean():.6f}, {dev:.2f} sigma")
    assert dev <= 4.0


def test_seeds_0_and_1_are_unrelated():
    rows = np.arange(20000)[:, None]
    feats = np.arange(256)[None, :]
    agree = (keep_mask(0.5, 0, rows, feats) == keep_mask(0.5, 1, rows, feats)).mean()
    print(f"seeds 0 and 1 agree on {agree:.4%}")
    assert 0.49 <= agree <= 0.51
    # seeds that differ only in the high word
    agree = (keep_mask(0.5, 5, rows, feats) == keep_mask(0.5, 5 + 2 ** 32, rows, feats)).mean()
    assert 0.49 <= agree <= 0.51


def test_mask_is_keyed_on_the_global_row():
    feats = np.arange(256)[None, :]
    full = keep_mask(0.5, 77, np.arange(67)[:, None], feats)
    part = keep_mask(0.5, 77, 20 + np.arange(30)[:, None], feats)
    assert np.array_equal(part, full[20:50])
    assert not keep_mask(1.0, 77, np.arange(8)[:, None], feats).any()
    assert keep_mask(0.0, 77, np.arange(8)[:, None], feats).all()


# ------------------------------------------------------------------ the C entry points
def test_header_declares_and_binding_binds_the_dropout_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("maxk_topk_cbsr_dropout", "maxk_scatter_backward_dropout"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
    assert _lib.lib.maxk_abi_version() == 4      # new symbols only


def _topk(records=None, record_bytes=0, layout=0, k=16, d=256, n=10, p=0.5, row_offset=0,
          tables=False):
    sd = P(8192) if tables else None
    si = P(16384) if tables else None
    rc = _lib.lib.maxk_topk_cbsr_dropout(None, records, record_bytes, layout, sd, 0, si, 0, None,
                                         None, None, 0, n, d, k, 0, p, 12345, row_offset, None)
    return rc, _lib.lib.maxk_last_error().decode()


def _scatter(p=0.5, row_offset=0, n=10):
    rc = _lib.lib.maxk_scatter_backward_dropout(None, None, 0, None, n, 256, 16, p, 12345,
                                                row_offset, None)
    return rc, _lib.lib.maxk_last_error().decode()


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan"), float("inf")])
def test_probability_out_of_range_is_refused(p):
    rc, msg = _topk(P(4096), 128, 4, p=p)
    assert rc == INVALID and "maxk_topk_cbsr_dropout" in msg and "p must" in msg
    rc, msg = _scatter(p=p)
    assert rc == INVALID and "maxk_scatter_backward_dropout" in msg and "p must" in msg


def test_negative_row_offset_is_refused():
    for p in (0.0, 0.5):
        rc, msg = _topk(P(4096), 128, 4, p=p, row_offset=-1)
        assert rc == INVALID and "maxk_topk_cbsr_dropout" in msg and "row_offset" in msg
        rc, msg = _scatter(p=p, row_offset=-1)
        assert rc == INVALID and "maxk_scatter_backward_dropout" in msg and "row_offset" in msg


# the record-argument cases of test_records_capi.py
@pytest.mark.parametrize("records,record_bytes,layout,k,code", [
    (P(4096 + 8), 128, 4, 16, INVALID),    # records not 16-B aligned
    (P(4096 + 4), 64, 2, 8, INVALID),
    (P(4096), 136, 4, 16, INVALID),        # record_bytes no multiple of 16
    (P(4096), 112, 4, 16, INVALID),        # 8 pair chunks need 128 B
    (P(4096), 32, 2, 8, INVALID),          # 3 lane chunks need 48 B
    (P(4096), 64, 1, 16, INVALID),         # layout 1 needs 5k = 80 B
    (P(4096), 256, 4, 15, INVALID),        # pair chunks need an even k
    (P(4096), 2048, 4, 130, INVALID),      # 65 pair chunks
    (P(4096), 2048, 2, 193, INVALID),      # 65 lane chunks
    (P(4096), 128, 1, 18, INVALID),        # layout 1 needs k % 4 == 0
    (P(4096), 128, 5, 16, UNSUPPORTED),    # no such layout
    (P(4096), 128, 0, 16, UNSUPPORTED),
    (P(4096), 128, 3, 16, UNSUPPORTED),
])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_record_argument_errors(records, record_bytes, layout, k, code, p):
    rc, msg = _topk(records, record_bytes, layout, k, p=p)
    assert rc == code, msg
    assert "maxk_topk_cbsr_dropout" in msg


@pytest.mark.parametrize("record_bytes,layout,k", [
    (128, 4, 16), (1024, 4, 128), (48, 2, 8), (16, 2, 1), (80, 1, 16),
])
def test_valid_record_arguments_pass_the_record_checks(record_bytes, layout, k):
    """Valid record arguments get past the checks: refused for the null input (N > 0), a
    no-op at N = 0."""
    rc, msg = _topk(P(4096), record_bytes, layout, k)
    assert rc == INVALID and "null pointer" in msg
    assert _topk(P(4096), record_bytes, layout, k, n=0)[0] == 0


def test_without_records_both_tables_are_required():
    rc, msg = _topk(None)                    # no records, no tables
    assert rc == INVALID and "maxk_topk_cbsr_dropout" in msg and "null" in msg
    rc, msg = _topk(None, tables=True)       # tables given: only the null input is left
    assert rc == INVALID and "null pointer" in msg
    # the layout is not looked at without records
    assert _topk(None, 0, 7, tables=True, n=0)[0] == 0


def test_empty_input_is_a_no_op():
    assert _topk(None, n=0)[0] == 0
    assert _topk(None, n=0, p=0.0)[0] == 0
    assert _topk(None, n=0, p=1.0)[0] == 0
    assert _scatter(n=0)[0] == 0 and _scatter(n=0, p=0.0)[0] == 0


def test_scatter_null_pointers_are_refused_on_the_host():
    rc, msg = _scatter()
    assert rc == INVALID and "null pointer" in msg
