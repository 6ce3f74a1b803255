"""Helpers of the CSR-transposition tests (tests/test_transpose_capi.py, tests/test_gpu_transpose.py):
the numpy restatement of the rule of include/maxk_hip.h ("CSR transposition"), the digit plan and
the scratch size restated, the kernel names of a call, and the input cases."""
import functools
import os
import re

import numpy as np

import gat_heads as gh
import sampling as sp
import scan

# csrc/variants_transpose.h, asserted against the header's text by tests/test_transpose_capi.py
WAVE = 64                 # kTrWave: items a wave ranks at a time
SUB_RUN = 2048            # kTrSubRun: consecutive items of one wave
TILE = 8192               # kTrTile: items of a work-group
MAX_DIGIT_BITS = 11       # kTrMaxDigitBits
MAX_PASSES = 3            # kTrMaxPasses
SCAN_TILE = scan.TILE     # items of a scan tile (csrc/scan.h)
HEADER_CONSTANTS = {"kTrWave": WAVE, "kTrSubRun": SUB_RUN, "kTrTile": TILE,
                    "kTrMaxDigitBits": MAX_DIGIT_BITS, "kTrMaxPasses": MAX_PASSES}
SIZES = (WAVE, SUB_RUN, TILE)     # E at each of these - 1, at, + 1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = os.path.join(ROOT, "spgemm-gnn_amd", "csrc", "variants_transpose.h")

SCAN_KERNELS = scan.PLAIN_KERNELS                          # both scans are the plain one
COMMON_KERNELS = SCAN_KERNELS + ("maxk_tr::zero_kernel",)  # and the one fill: in every call
FIRST, MIDDLE, LAST, ONLY = 0, 1, 2, 3


def header_constants():
    """The constants above as csrc/variants_transpose.h evaluates them."""
    text = open(VARIANTS).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (kTr\w+) = ([^;]+);", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))  # noqa: S307 (arithmetic)
    return env


# ------------------------------------------------------------------ the rule
def transpose_ref(ptr, idx, num_cols, val=None):
    """(out_ptr, out_row, out_order[, out_val]): out_order ascends in (c(e), e) with c the clamped
    column, out_row[j] is the row whose range holds edge out_order[j], out_ptr the exclusive scan
    of the column counts, out_val the values in that order (bits untouched)."""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    c = np.clip(idx, 0, max(num_cols - 1, 0))
    order = np.lexsort((np.arange(idx.size), c))
    row = np.searchsorted(ptr, order, side="right") - 1
    out_ptr = np.zeros(num_cols + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=num_cols)[:num_cols], out=out_ptr[1:])
    out = (out_ptr.astype(np.int32), row.astype(np.int32), order.astype(np.int32))
    return out if val is None else out + (np.asarray(val)[order],)


# ------------------------------------------------------------------ digit plan, scratch
def key_bits(num_cols):
    return max(int(num_cols) - 1, 0).bit_length()


def digit_bits(num_cols):
    """The digit widths of the passes, lowest digit first."""
    b = key_bits(num_cols)
    p = max(1, -(-b // MAX_DIGIT_BITS))
    return tuple(b // p + (1 if i < b % p else 0) for i in range(p))


def scratch_bytes(num_rows, num_cols, num_edges):
    if num_edges == 0:
        return 0
    widths = digit_bits(num_cols)
    pairs = 8 * num_edges if len(widths) > 1 else 0
    hist = -(-num_edges // TILE) << widths[0]
    return pairs + 4 * (hist + -(-max(hist, num_cols + 1) // SCAN_TILE))


def kernels(num_cols, has_val):
    """The maxk_tr:: and maxk_scan:: kernels one call with edges launches."""
    p = len(digit_bits(num_cols))
    names = set(COMMON_KERNELS) | {"maxk_tr::tile_hist_kernel<true>"}
    if p > 1:
        names.add("maxk_tr::tile_hist_kernel<false>")
    v = "true" if has_val else "false"
    roles = [(ONLY, v)] if p == 1 else [(FIRST, "false"), (LAST, v)] + \
        ([(MIDDLE, "false")] if p == 3 else [])
    return names | {f"maxk_tr::scatter_pass_kernel<{r}, {b}>" for r, b in roles}


def pass_kernel_names():
    """Every instantiation of the two variant tables, as tools/variant_check.cpp prints them."""
    names = set()
    for nc in (1, 2 ** MAX_DIGIT_BITS + 1, 2 ** (2 * MAX_DIGIT_BITS) + 1):
        for v in (False, True):
            names |= kernels(nc, v) - set(COMMON_KERNELS)
    return names


# ------------------------------------------------------------------ inputs
def random_csr(num_rows, num_cols, num_edges, seed):
    """(ptr, idx, num_cols): random row lengths (empty rows included) and random columns."""
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.integers(0, num_rows, num_edges))
    ptr = np.zeros(num_rows + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=num_rows), out=ptr[1:])
    idx = rng.integers(0, num_cols, num_edges)
    return ptr.astype(np.int32), idx.astype(np.int32), num_cols


def transpose_of(ptr, idx, num_cols):
    ptr_t, idx_t, _ = transpose_ref(ptr, idx, num_cols)
    return ptr_t, idx_t, ptr.size - 1


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ptr, idx, num_cols). The 600-row graph (about 17k edges: three tiles) and the
    300 x 900 one of tests/sampling.py, both again as their own transposes; no edges; one row; one
    column that holds every edge of three tiles and a bit; E around every size of SIZES; columns
    out of range."""
    out = {"square": sp.square_graph(), "rect": sp.rect_graph()}
    out["square_t"] = transpose_of(*out["square"])
    out["rect_t"] = transpose_of(*out["rect"])
    out["no_edges"] = (np.zeros(41, np.int32), np.zeros(0, np.int32), 40)
    e1 = 3 * TILE + 100
    out["one_row"] = (np.array([0, e1], np.int32),
                      np.random.default_rng(3).integers(0, 5000, e1).astype(np.int32), 5000)
    p, _, _ = random_csr(700, 1, e1, 4)
    out["one_column"] = (p, np.zeros(e1, np.int32), 1)
    out["one_hub_column"] = (p, np.full(e1, 2600, np.int32), 5000)
    for t in SIZES:
        for e in (t - 1, t, t + 1):
            out[f"edges_{e}"] = random_csr(300, 5000, e, e)
    ptr, idx, nc = random_csr(200, 3000, 6000, 8)
    idx = idx.copy()
    idx[::7] = nc + np.arange(idx[::7].size)
    idx[3::11] = -1 - np.arange(idx[3::11].size)
    idx[5], idx[6] = 2 ** 31 - 1, -2 ** 31
    out["stray_columns"] = (ptr, idx, nc)
    for arrays in out.values():
        for a in arrays[:2]:
            a.setflags(write=False)
    return out


def column_counts():
    """num_cols of the digit-plan cases: 1, 2, 3, and 2^b - 1, 2^b, 2^b + 1 for every b at which
    the plan changes its pass count or a width (every b: the key grows by a bit at 2^b + 1), up to
    the first num_cols that reaches the largest pass count."""
    out, b = {1, 2, 3}, 1
    while True:
        out |= {2 ** b - 1, 2 ** b, 2 ** b + 1}
        if len(digit_bits(2 ** b + 1)) == MAX_PASSES:
            return sorted(out)
        b += 1


def plan_case(num_cols, num_edges=3000):
    """(ptr, idx, num_cols) of about 3,000 edges whose columns include 0, the last column and
    both sides of every digit boundary of the plan, besides random ones."""
    ptr, idx, _ = random_csr(150, num_cols, num_edges, num_cols % 1000 + 7)
    must, shift = [0, num_cols - 1], 0
    for w in digit_bits(num_cols)[:-1]:
        shift += w
        must += [c for c in ((1 << shift) - 1, 1 << shift, (1 << shift) + 1) if c < num_cols]
    idx = idx.copy()
    for i, c in enumerate(must * 3):                     # each more than once, apart
        idx[(i * 97 + 11) % idx.size] = c
    assert set(must) <= set(idx.tolist())
    return ptr, idx, num_cols


def values(num_edges, seed=0):
    """f32 [E] of random bit patterns (NaNs with payloads, denormals, both infinities among
    them), the special values first. Compare as bits."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, num_edges, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
                        0x7F800001, 0xFFBFFFFF, 0x00000001, 0x807FFFFF, 0x3F800000], np.uint32)
    bits[:min(special.size, num_edges)] = special[:num_edges]
    return bits.view(np.float32)
