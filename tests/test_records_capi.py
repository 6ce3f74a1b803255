"""CPU: the record entry points (maxk_topk_cbsr_records, maxk_spgemm_forward_records) are
declared, bound, and refuse bad record arguments on the host, before any device call."""
import ctypes
import os
import re

import pytest

from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -2


def test_header_declares_and_binding_binds_the_record_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("maxk_topk_cbsr_records", "maxk_spgemm_forward_records"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
    # same version: appended fields and new symbols only
    assert _lib.lib.maxk_abi_version() == 4
    assert "#define MAXK_ABI_VERSION 4" in open(HEADER).read()


def test_plan_info_ends_with_fwd_fixed():
    names = [f[0] for f in _lib.PlanInfo._fields_]
    assert names[-3:] == ["fwd_layout", "fwd_record_bytes", "fwd_fixed"]
    assert ctypes.sizeof(_lib.PlanInfo._fields_[-1][1]) == 4


def _topk_records(records, record_bytes, layout, k, d=256, n=10):
    rc = _lib.lib.maxk_topk_cbsr_records(None, records, record_bytes, layout, None, 0, None, 0,
                                         None, None, None, 0, n, d, k, 0, None)
    return rc, _lib.lib.maxk_last_error().decode()


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
def test_topk_records_argument_errors(records, record_bytes, layout, k, code):
    rc, msg = _topk_records(records, record_bytes, layout, k)
    assert rc == code, msg
    assert "maxk_topk_cbsr_records" in msg


@pytest.mark.parametrize("record_bytes,layout,k", [
    (128, 4, 16), (144, 4, 16), (1024, 4, 128), (48, 2, 8), (16, 2, 1), (1024, 2, 192),
    (80, 1, 16), (128, 1, 16),
])
def test_topk_records_valid_record_arguments_pass_the_record_checks(record_bytes, layout, k):
    """The same calls with valid record arguments get past them: refused for the null input
    (N > 0), accepted as a no-op at N = 0."""
    rc, msg = _topk_records(P(4096), record_bytes, layout, k)
    assert rc == INVALID and "null pointer" in msg
    rc, _ = _topk_records(P(4096), record_bytes, layout, k, n=0)
    assert rc == 0
    rc, msg = _topk_records(None, record_bytes, layout, k)
    assert rc == INVALID and "maxk_topk_cbsr_records" in msg and "null" in msg


def test_forward_records_rejects_null_plan_and_bad_flags():
    lib = _lib.lib
    rc = lib.maxk_spgemm_forward_records(None, None, None, None, P(4096), 128, 4, None, 10, 100,
                                         16, 256, 0, None, 0, 0, None)
    assert rc == INVALID
    assert "maxk_spgemm_forward_records" in lib.maxk_last_error().decode()
    rc = lib.maxk_spgemm_forward_records(None, None, None, None, P(4096), 128, 4, None, 10, 100,
                                         16, 256, 2, None, 0, 0, None)
    assert rc == INVALID and "accumulate" in lib.maxk_last_error().decode()
