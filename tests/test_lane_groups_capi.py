"""The argument checks that the multi-head and the max aggregation share (csrc/lane_groups.h,
check_shape), on the host: every refusal's code and full text, and the order in which two
refusals of one call fire. The texts are literals, copied from the two operators' sources as they
stood before the checks were shared; the same table passes against a library of that revision."""
import ctypes

import pytest

from maxk_kernels import _lib

P = ctypes.c_void_p
lib = _lib.lib
INVALID, UNSUPPORTED = -1, -2
I32MAX = 2 ** 31 - 1
SOME = P(1 << 20)        # a non-null pointer that no refusal dereferences


def heads_fwd(out=None, ds=0, is_=0, H=4, n=10, nc=10, e=100, D=256, k=16):
    return lib.maxk_heads_aggregate_forward(None, None, None, None, ds, None, is_, out, H, n, nc,
                                            e, D, k, None)


def heads_bwd(gsp=SOME, ga=None, gs=0, ds=0, is_=0, H=4, n=10, nc=10, e=100, D=256, k=16):
    return lib.maxk_heads_aggregate_backward(None, None, None, None, None, gs, None, ds, None, is_,
                                             gsp, ga, H, n, nc, e, D, k, None)


def max_fwd(out=None, ae=None, sl=None, ds=0, is_=0, n=10, nc=10, e=100, D=256, k=16):
    return lib.maxk_max_aggregate_forward(None, None, None, ds, None, is_, out, ae, sl, n, nc, e,
                                          D, k, None)


def max_bwd(gsp=None, gs=0, is_=0, n=10, nc=10, e=100, D=256, k=16):
    return lib.maxk_max_aggregate_backward(None, None, None, None, gs, None, None, None, is_, gsp,
                                           n, nc, e, D, k, None)


CALLS = {"maxk_heads_aggregate_forward": heads_fwd, "maxk_heads_aggregate_backward": heads_bwd,
         "maxk_max_aggregate_forward": max_fwd, "maxk_max_aggregate_backward": max_bwd}
HEADS = tuple(n for n in CALLS if "heads" in n)
FORWARD = tuple(n for n in CALLS if "forward" in n)
BACKWARD = tuple(n for n in CALLS if "backward" in n)

SIZES = "sizes out of range"
DIM = "dim_origin must be in [1, 256]"
K = "k must be between 1 and input dimension"
DS = "data_stride must be >= k (0: k)"
IS = "index_stride must be >= k (0: k)"
GS = "grad_stride must be >= dim_origin (0: dim_origin)"
NO_COLS = "sizes out of range: edges without columns"
NO_ROWS = "sizes out of range: edges without rows"
NULL = "null pointer"
H_DIV = "num_heads must be >= 1 and divide dim_origin"
H_MUL4 = "dim_origin / num_heads must be a multiple of 4"
H_MAX = "num_heads above 16 is not supported"
BOTH = "arg_edge and arg_slot must both be given or both be NULL"

# (entry points, arguments, code, text). With two faults in one call the text is the one of the
# check that comes first: sizes, dim_origin, k, heads, data_stride (heads), index_stride, edges
# without columns, without rows, then data_stride and arg_* (max forward), grad_stride
# (backward), null output.
TABLE = [
    (CALLS, dict(n=-1), INVALID, SIZES), (CALLS, dict(nc=-1), INVALID, SIZES),
    (CALLS, dict(e=-1), INVALID, SIZES), (CALLS, dict(e=I32MAX + 1), INVALID, SIZES),
    (CALLS, dict(n=-1, D=0), INVALID, SIZES),
    (CALLS, dict(D=0), INVALID, DIM), (CALLS, dict(D=257, k=300), INVALID, DIM),
    (CALLS, dict(k=0), INVALID, K), (CALLS, dict(D=8, k=9), INVALID, K),
    (CALLS, dict(k=0, is_=-1, nc=0), INVALID, K),
    (HEADS, dict(H=0), INVALID, H_DIV), (HEADS, dict(H=3), INVALID, H_DIV),
    (HEADS, dict(H=0, k=0), INVALID, K),
    (HEADS, dict(D=40, H=20, k=8), UNSUPPORTED, H_MUL4),
    (HEADS, dict(D=136, H=17, k=8), UNSUPPORTED, H_MAX),
    (HEADS, dict(D=34, H=17, k=8), UNSUPPORTED, H_MUL4),
    (HEADS, dict(H=3, ds=1), INVALID, H_DIV),
    (HEADS, dict(ds=15), INVALID, DS), (HEADS, dict(ds=15, is_=15), INVALID, DS),
    (CALLS, dict(is_=15), INVALID, IS), (CALLS, dict(is_=15, nc=0), INVALID, IS),
    (CALLS, dict(nc=0), INVALID, NO_COLS), (CALLS, dict(nc=0, n=0), INVALID, NO_COLS),
    (CALLS, dict(n=0), INVALID, NO_ROWS),
    (("maxk_max_aggregate_forward",), dict(ds=15), INVALID, DS),
    (("maxk_max_aggregate_forward",), dict(ds=15, is_=15), INVALID, IS),
    (("maxk_max_aggregate_forward",), dict(ds=15, n=0), INVALID, NO_ROWS),
    (("maxk_max_aggregate_forward",), dict(ds=15, ae=SOME), INVALID, DS),
    (("maxk_max_aggregate_forward",), dict(ae=SOME), INVALID, BOTH),
    (("maxk_max_aggregate_forward",), dict(sl=SOME), INVALID, BOTH),
    (BACKWARD, dict(gs=255), INVALID, GS), (BACKWARD, dict(gs=255, nc=0), INVALID, NO_COLS),
    (BACKWARD, dict(gs=255, gsp=None), INVALID, GS),
    (FORWARD, dict(), INVALID, NULL), (FORWARD, dict(e=0), INVALID, NULL),
    (("maxk_max_aggregate_backward",), dict(), INVALID, NULL),
    (("maxk_max_aggregate_backward",), dict(e=0), INVALID, NULL),
    (("maxk_heads_aggregate_backward",), dict(), INVALID, NULL),     # the inputs, grad_sp is given
]
CASES = [(name, kw, code, text) for names, kw, code, text in TABLE for name in names]


@pytest.mark.parametrize("name,kw,code,text", CASES)
def test_refusal_code_and_full_text(name, kw, code, text):
    got = CALLS[name](**kw)
    assert (got, lib.maxk_last_error().decode()) == (code, f"{name}: {text}")


def test_calls_that_are_not_refused():
    # nothing to do: no rows (columns), or no gradient asked for; no pointer is dereferenced
    assert heads_fwd(n=0, e=0) == 0 and max_fwd(n=0, e=0) == 0
    assert heads_bwd(nc=0, e=0) == 0 and max_bwd(nc=0, e=0) == 0
    assert heads_bwd(gsp=None) == 0
