"""The launchers' dispatch restated, and one case per compiled kernel instantiation (a plain
module, no tests: tests/test_kernel_variant_inputs.py checks what is built here on the CPU,
tests/test_gpu_kernel_variants.py launches every case).

tests/golden/kernel_instantiations.txt lists the kernel instantiations compiled into
libmaxk_hip.so (tools/kernel_list.py writes it, tests/test_kernel_list.py holds it to the built
library). The functions below return the fixture's exact name for a launch, from
`GraphPlan.info()` and the call's arguments, written from the launcher source:

forward_kernel          launch_spgemm_fwd (csrc/spgemm.hip): V, flags, threads, sub-steps, 4-byte words
forward_pass_kernels    spgemm_forward_impl before that launch: record packs, split-row zeroing,
                        statistics / pack pass (launch_cbsr_stats)
bwd_slots               choose_bwd_shape (csrc/plan.hip): F, S and the padded k, which info() does not
                        report, from the documented rules of maxk_plan_options (as sweep.expected)
column_block_kernel     sspmm_backward_impl, column blocks: U, threads, F, Q, big
row_pass_kernel         sspmm_backward_impl, two-pass row pass: rows per wavefront
topk_kernel             topk_impl (csrc/maxk_topk.hip), both modes
scatter_kernel          scatter_impl; sddmm_kernel: sddmm_impl; dense_spmm_kernel: maxk_dense_spmm_csr

SINGLES is the table of the kernels with one instantiation: the scenario that reaches each and
the fact (from info() or the call) that shows it did. `cases()` is the list of cases; every
fixture name is the target of at least one.

Inputs follow tests/sweep.py: integer features and gradients, edge values from {0.5, 1, 2},
dropout p = 0.5, so every sum is exact in f32 in any order and the GPU cases compare with
np.array_equal.
"""
import collections
import functools
import os
import types

import numpy as np

import rowconst
import sweep
from oracle import oracle
from structured import int_features

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations.txt")
D = 256
WAVE = 64
LDS_BYTES = sweep.LDS_BYTES
TOPK_ROWS8 = 1 << 20               # rows from which the plain exact top-k takes 8 rows per wave
NS = "maxk::"


def fixture_names():
    with open(FIXTURE) as f:
        return [ln.strip() for ln in f if ln.strip()]


def _b(v):
    return "true" if v else "false"


def _name(kernel, *params):
    return NS + kernel + "<" + ", ".join(_b(p) if isinstance(p, (bool, np.bool_)) else str(p)
                                        for p in params) + ">"


# ---------------------------------------------------------------------------- forward
def fwd_lanes(layout, k):
    """Lanes per edge: ceil(k / 3) lane chunks, k / 2 pair chunks, else k / 4."""
    return (k + 2) // 3 if layout == 2 else k // 2 if layout == 4 else k // 4


def forward_kernel(info):
    """spgemm_fwd_kernel<V, FL, NT, FU, RC> of a plan: V = 1 for fwd_layout 3 (one feature per
    lane), else 4; FL = 1 lane chunks | 4 pair chunks | 2 quad-shared edge words (fixed point
    and the lanes of an edge a multiple of 4); 8 waves run 512 threads, 4 waves 256; 4 sub-steps
    only with 8 waves and never with 4-byte words (RC)."""
    k, layout = info["dim_k"], info["fwd_layout"]
    if layout == 3:
        v, fl = 1, 0
    else:
        v = 4
        quad = bool(info["fwd_fixed"]) and fwd_lanes(layout, k) % 4 == 0
        fl = (1 if layout == 2 else 0) | (4 if layout == 4 else 0) | (2 if quad else 0)
    rc = bool(info["fwd_rowconst"])
    nt = 512 if info["fwd_waves"] == 8 else 256
    fu = 4 if not rc and info["fwd_waves"] == 8 and info["fwd_unroll"] == 4 else 8
    return _name("spgemm_fwd_kernel", v, fl, nt, fu, rc)


def forward_pass_kernels(info, stats_given=False):
    """What GraphPlan.forward(sp_data, sp_index) on two plain tables launches before the forward
    kernel, in launch order: the chunk-record pack (lane chunks; pair chunks when k % 4 != 0), the
    zeroing of split rows when no statistics / pack pass of k % 4 == 0 does it, and that pass:
    cbsr_stats4_kernel<PACK, STATS> with PACK 2 pair chunks, 1 packed records, 0 none, STATS the
    fixed-point pair (always with PACK 0); cbsr_stats_kernel when k % 4 != 0."""
    k, layout = info["dim_k"], info["fwd_layout"]
    st = bool(info["fwd_fixed"]) and not stats_given
    out = []
    if layout == 2:
        out.append(_name("pack_cbsr3_kernel", 3))
    elif layout == 4 and k % 4:
        out.append(_name("pack_cbsr3_kernel", 2))
    pack4 = layout in (1, 4) and k % 4 == 0
    if info["fwd_split_rows"] and not ((pack4 or st) and k % 4 == 0):
        out.append(NS + "zero_rows_kernel")
    if pack4 or st:
        if k % 4 == 0:
            pk = (2 if layout == 4 else 1) if pack4 else 0
            out.append(_name("cbsr_stats4_kernel", pk, st if pack4 else True))
        else:
            out.append(NS + "cbsr_stats_kernel")
    return out


# ---------------------------------------------------------------------------- backward
def bwd_slots(k, opts, n_rows, n_cols, edges):
    """(F, S, padded k) of a plan's column-block backward, from maxk_plan_options'
    bwd_features_per_lane and bwd_slot_groups: F = 2 by default at k = 8 below 10 edges per
    block row, for k % 4 == 2 up to 128 and at k = 16 with two slot groups, else 4 (2 above k =
    128 runs 4); k is padded to a multiple of F; S = 2 by default from k = 16 with k % 8 == 0
    below 4.5 edges per block row, halved until F x S divides the padded k."""
    lds = opts.get("bwd_lds_bytes", 0) or LDS_BYTES

    def per_block_row(kk):
        return edges / n_rows * min(float(n_cols), (lds - 16) / (5.0 * kk)) / n_cols

    fpl, sg = opts.get("bwd_features_per_lane", 0), opts.get("bwd_slot_groups", 0)
    live = n_rows > 0 and n_cols > 0
    two = k == 8 and live and per_block_row(8) < 10.0
    f = fpl or (2 if two or (k % 4 == 2 and k <= 2 * WAVE) else 4)
    if f == 2 and (k + 1) // 2 > WAVE:
        f = 4
    kp = -(-k // f) * f
    s = sg or 1
    if sg == 0 and f == 4 and k >= 16 and k % 8 == 0 and live and per_block_row(k) < 4.5:
        s = 2
    while s > 1 and kp % (f * s):
        s //= 2
    if fpl == 0 and f == 4 and s == 2 and kp // s == 8:
        f = 2
    return f, s, kp


def column_block_kernel(info, f, s, kp):
    """sspmm_bwd4_kernel<U, NT, F, Q, BIG>: Q when the lanes of an edge, (padded k / S) / F, are
    a multiple of 4; BIG when grad_out (num_nodes x dim_origin floats) exceeds 32-bit byte
    offsets, which runs 8 waves x 8 sub-steps; else the shape info() reports: 16 waves x 8, 12 x
    12 or 8, 8 x 16, 12 or 8."""
    lanes = kp // s // f
    big = info["num_nodes"] * info["dim_origin"] * 4 > 0xFFFFFFFF
    w, u = info["bwd_waves"], info["bwd_unroll"]
    if big:
        shape = (8, 512)
    elif w == 16:
        shape = (8, 1024)
    elif w == 12:
        shape = (12, 768) if u == 12 else (8, 768)
    else:
        shape = (16, 512) if u == 16 else (12, 512) if u == 12 else (8, 512)
    return _name("sspmm_bwd4_kernel", shape[0], shape[1], f, lanes % 4 == 0, big)


def row_pass_kernel(n_rows, edges):
    """sspmm_bwd_rows_kernel<4, R>: R destination rows per wavefront, doubled from 1 up to 4
    while a wavefront would see fewer than 256 edges."""
    r = 1
    while r < 4 and r * edges / max(n_rows, 1) < 256.0:
        r *= 2
    return _name("sspmm_bwd_rows_kernel", 4, r)


# ---------------------------------------------------------------------------- top-k, scatter
def topk_kernel(mode, n, d, k, stats=False, records=False, dropout=False, dense=False):
    """exact: topk_exact_kernel<rows per wave, k > 64, D == 256, stats, rec, drop, dense>; the
    dropout and dense kernels are record kernels (the record is optional at run time); 8 rows
    per wave only for the plain top-k of k <= 64 from 2^20 rows; a dense partial row with
    statistics takes the k > 64 kernel at every k. ref_compat:
    topk_ref_compat_kernel<D == 256, stats, rec, drop, dense>."""
    full, wide = d == 4 * WAVE, k > WAVE
    if mode == "exact":
        if dense:
            w = wide or (not full and stats)
            return _name("topk_exact_kernel", 4, w, full, stats, True, dropout, True)
        if dropout:
            return _name("topk_exact_kernel", 4, wide, full, stats, True, True, False)
        if not (wide or n < TOPK_ROWS8 or stats or records):
            return _name("topk_exact_kernel", 8, False, full, False, False, False, False)
        return _name("topk_exact_kernel", 4, wide, full, stats, records, False, False)
    assert mode == "ref_compat", mode
    if dense:
        return _name("topk_ref_compat_kernel", full, stats, True, dropout, True)
    if dropout:
        return _name("topk_ref_compat_kernel", full, stats, True, True, False)
    return _name("topk_ref_compat_kernel", full, stats, records, False, False)


def scatter_kernel(dropout=False, merge=False):
    return _name("maxk_scatter_backward_kernel", dropout, merge)


def sddmm_kernel(k):
    """sddmm_edge_grad_kernel<lanes per edge>: k rounded up to a power of two, over 4."""
    k2 = 1
    while k2 < k:
        k2 <<= 1
    return _name("sddmm_edge_grad_kernel", k2 // 4 if k2 >= 4 else 1)


def dense_spmm_kernel(d):
    """dense_spmm_kernel<L, 4>: L lanes per row for D / 4 float4 columns."""
    c4 = d // 4
    return _name("dense_spmm_kernel", 64 if c4 > 32 else 32 if c4 > 16 else 16 if c4 > 8 else
                 8 if c4 > 4 else 4, 4)


# ---------------------------------------------------------------------------- single instances
# kernel -> (scenario of tests/test_gpu_kernel_variants.py, why the scenario launches it, the
# fact that shows it: a predicate over the scenario's facts, mostly its plan's info())
def _always(f):
    return True


SINGLES = {
    # plan build, every plan with edges
    "expand_rows_kernel": ("column_blocks", "row id of every CSR edge: any build with edges",
                           lambda f: f["info"]["num_edges"] > 0),
    "fwd_key_kernel": ("column_blocks", "the forward's permuted sort: any build with edges",
                       lambda f: f["info"]["fwd_tasks"] > 0 and f["info"]["num_edges"] > 0),
    "gather_fwd_kernel": ("column_blocks", "the forward's edge words: any build with edges",
                          lambda f: f["info"]["fwd_tasks"] > 0 and f["info"]["num_edges"] > 0),
    "fwd_phase_kernel": ("column_blocks", "column-window offsets: any build with forward tasks",
                         lambda f: f["info"]["fwd_tasks"] > 0),
    "fwd_row_sums_kernel": ("column_blocks", "fixed-point bounds: a build with fwd_fixed",
                            lambda f: f["info"]["fwd_fixed"] == 1),
    "fwd_fix_stats_kernel": ("column_blocks", "fixed-point bounds: a build with fwd_fixed",
                             lambda f: f["info"]["fwd_fixed"] == 1),
    # column blocks
    "bwd_key_kernel": ("column_blocks", "block sort with ascending rows (bwd_row_order 1)",
                       lambda f: f["info"]["bwd_algo"] == 1 and f["info"]["bwd_row_order"] == 1),
    "key_offsets_kernel": ("column_blocks", "block offsets of the sorted edges",
                           lambda f: f["info"]["bwd_blocks"] >= 1),
    "gather_bwd_kernel": ("column_blocks", "rows / block positions of the reordered edges",
                          lambda f: f["info"]["bwd_algo"] == 1),
    "gather_i32_kernel": ("column_blocks", "first rows of the chunks: column-block tasks",
                          lambda f: f["info"]["bwd_algo"] == 1 and f["info"]["bwd_tasks"] > 0),
    "build_bwd_rec_kernel": ("column_blocks", "the column blocks' edge records",
                             lambda f: f["info"]["bwd_algo"] == 1 and f["info"]["bwd_tasks"] > 0),
    "bwd_key64_kernel": ("row_order_2", "bwd_row_order = 2: 64-bit {block, row} keys",
                         lambda f: f["info"]["bwd_row_order"] == 2),
    "key_block_kernel": ("row_order_2", "bwd_row_order = 2: block ids of the 64-bit keys",
                         lambda f: f["info"]["bwd_row_order"] == 2),
    "dense_window_kernel": ("auto_row_order", "automatic row order, column blocks, >= 2048 edges",
                            lambda f: f["info"]["bwd_algo"] == 1 and f["opts"].get(
                                "bwd_row_order", 0) == 0 and f["info"]["num_edges"] >= 2048),
    "affine_order_kernel": ("scattered", "col_order = scattered",
                            lambda f: f["info"]["col_order"] == 2),
    "invert_order_kernel": ("scattered", "col_order = scattered: column -> position",
                            lambda f: f["info"]["col_order"] == 2),
    "iota_kernel": ("identity_order", "maxk_plan_get_col_order of a plan without an order",
                    lambda f: f["info"]["col_order"] == 1),
    "bwd_combine_kernel": ("slab_flush", "column blocks split over work-groups, slab flush",
                           lambda f: f["info"]["bwd_shared_blocks"] > 0 and
                           f["opts"].get("bwd_flush", 0) in (0, 2)),
    # two-pass
    "build_erec_kernel": ("two_pass_chunks", "two-pass edge records",
                          lambda f: f["info"]["bwd_algo"] == 3),
    "sspmm_bwd_cols_kernel<4>": ("two_pass_chunks", "two-pass column pass",
                                 lambda f: f["info"]["bwd_algo"] == 3),
    "tp_colptr_kernel": ("two_pass_chunks", "two-pass with more than one row chunk",
                         lambda f: f["info"]["bwd_algo"] == 3 and f["info"]["bwd_tp_chunks"] > 1),
    # forward edge words
    "fwd_rowconst_kernel": ("value_refresh", "row-constancy test: a build whose forward has the "
                            "4-byte form", lambda f: f["rowconst"][0] == 1),
    "fwd_cv_narrow_kernel": ("value_refresh", "row-constant values at build, and a refresh from "
                             "mixed values back to row-constant ones",
                             lambda f: f["rowconst"] == [1, 0, 1]),
    "fwd_cv_widen_kernel": ("value_refresh", "a refresh from row-constant to mixed values",
                            lambda f: f["rowconst"][:2] == [1, 0]),
    "zero_rows_kernel": ("split_rows", "split rows and no statistics / pack pass of k % 4 == 0",
                         lambda f: NS + "zero_rows_kernel" in forward_pass_kernels(f["info"])),
    "cbsr_stats_kernel": ("stats_odd_k", "maxk_cbsr_stats with k % 4 != 0", lambda f: f["k"] % 4),
    # top-k
    "fill_i32_kernel": ("topk_count", "exact top-k with a count output",
                        lambda f: f["mode"] == "exact" and f["count"]),
    "topk_stats_reduce_kernel": ("topk_count", "top-k with the fused statistics pair",
                                 lambda f: f["stats"]),
    # attention
    "edge_softmax_fwd_kernel": ("edge_softmax", "maxk_edge_softmax_forward", _always),
    "edge_softmax_bwd_kernel": ("edge_softmax", "maxk_edge_softmax_backward", _always),
    "gat_attention_fwd_kernel": ("gat_attention", "maxk_gat_attention_forward", _always),
    "gat_attention_bwd_kernel": ("gat_attention", "maxk_gat_attention_backward", _always),
    "edge_colsum_kernel": ("gat_attention", "maxk_edge_colsum", _always),
}
SINGLES = {NS + k: v for k, v in SINGLES.items()}


# ---------------------------------------------------------------------------- references
def sspmm_ref(rows, idx, val, g_rows, oi, with_mag=False):
    """grad_sp f64 [num_cols, k] of a rectangular graph given edge by edge: edge e goes from
    column idx[e] to the row whose gradient is g_rows[rows[e]]:
    grad_sp[c, j] = sum over the edges of c of val[e] * g[row(e), oi[c, j]]."""
    idx = np.asarray(idx, np.int64)
    terms = np.asarray(val, np.float64)[:, None] * \
        np.asarray(g_rows, np.float64)[np.asarray(rows, np.int64)[:, None], oi[idx]]
    out = np.zeros(oi.shape, np.float64)
    np.add.at(out, idx, terms)
    if not with_mag:
        return out
    mag = np.zeros(oi.shape, np.float64)
    np.add.at(mag, idx, np.abs(terms))
    return out, mag


def _values(rs, n):
    return rs.choice(np.array([0.5, 1.0, 2.0], np.float32), n).astype(np.float32)


# two-pass row pass: 50 rows x 600 columns with `deg` edges in every row
TP_ROWS, TP_COLS, TP_K = 50, 600, 16
TP_DEGREES = {1: 300, 2: 150, 4: 20}        # rows per wavefront -> edges per row


@functools.lru_cache(maxsize=None)
def tp_case(deg):
    rs = np.random.RandomState(5000 + deg)
    ptr = (np.arange(TP_ROWS + 1) * deg).astype(np.int32)
    idx = np.concatenate([np.sort(rs.randint(0, TP_COLS, deg)) for _ in range(TP_ROWS)])
    idx = idx.astype(np.int32)
    val = _values(rs, idx.size)
    g = int_features(TP_ROWS, D, seed=5100 + deg)
    oi = oracle.maxk(int_features(TP_COLS, D, seed=5200), TP_K, "exact")[1]
    rows = np.repeat(np.arange(TP_ROWS), deg)
    bwd, mag = sspmm_ref(rows, idx, val, g, oi, with_mag=True)
    return types.SimpleNamespace(p=ptr, ix=idx, v=val, n=TP_ROWS, nc=TP_COLS, k=TP_K, g=g, oi=oi,
                                 bwd=bwd, bwd_mag=mag)


# grad_out above 4 GiB: the rows of a 4,194,344 x 300 graph that carry edges
BIG_N = 4_194_304 + 40                      # N x 256 x 4 = 2^32 + 40960
BIG_COLS = 300
BIG_BOUNDARY = 4_194_304                    # first row whose byte offset needs 33 bits
BIG_ROWS = np.concatenate([np.arange(0, 24), np.arange(BIG_BOUNDARY - 12, BIG_BOUNDARY + 12),
                           np.arange(BIG_N - 24, BIG_N)]).astype(np.int64)
BIG_FQ = {(4, True): 16, (4, False): 10, (2, True): 8, (2, False): 6}     # (F, Q) -> k


@functools.lru_cache(maxsize=None)
def big_case(k):
    """ptr is returned as the touched rows and their degrees (the GPU case expands it on the
    device side of the transfer: 4.2 M int32); g holds the touched rows' gradients only."""
    rs = np.random.RandomState(6000 + k)
    deg = rs.randint(30, 51, BIG_ROWS.size)
    idx = np.concatenate([np.sort(rs.randint(0, BIG_COLS, d)) for d in deg]).astype(np.int32)
    val = _values(rs, idx.size)
    g = int_features(BIG_ROWS.size, D, seed=6100 + k)
    oi = oracle.maxk(int_features(BIG_COLS, D, seed=6200 + k), k, "exact")[1]
    local = np.repeat(np.arange(BIG_ROWS.size), deg)
    bwd, mag = sspmm_ref(local, idx, val, g, oi, with_mag=True)
    return types.SimpleNamespace(rows=BIG_ROWS, deg=deg, ix=idx, v=val, n=BIG_N, nc=BIG_COLS, k=k,
                                 g=g, oi=oi, bwd=bwd, bwd_mag=mag)


def big_ptr(c):
    """int32 [BIG_N + 1] CSR pointer of a big_case."""
    d = np.zeros(c.n, np.int64)
    d[c.rows] = c.deg
    ptr = np.zeros(c.n + 1, np.int64)
    np.cumsum(d, out=ptr[1:])
    return ptr.astype(np.int32)


@functools.lru_cache(maxsize=None)
def dense_spmm_case(d):
    """Y = A X on the sweep's sparse graph with integer X [600, d]: (x, y f64, sum of |terms|)."""
    p, ix, v = sweep.graph("sparse")
    x = int_features(sweep.N, d, seed=7000 + d)
    rows = np.repeat(np.arange(sweep.N), np.diff(p))
    terms = v.astype(np.float64)[:, None] * x[ix].astype(np.float64)
    y = np.zeros((sweep.N, d), np.float64)
    mag = np.zeros((sweep.N, d), np.float64)
    np.add.at(y, rows, terms)
    np.add.at(mag, rows, np.abs(terms))
    return x, y, mag


# attention: rows of power-of-two lengths whose logits are equal along the row, so the softmax is
# exactly 1 / length whatever the order of the sums; the gradients are integers
ATT_LENGTHS = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 1, 0, 64, 2, 256]
ATT_COLS = 97
ATT_SLOPE = 0.5


@functools.lru_cache(maxsize=None)
def attention_case():
    """ptr, per-row logits, idx / el / er of the GAT form and integer gradients. Row r takes
    columns of parity r % 2 only and el is 1 on even columns, 2 on odd ones, so el[idx] + er[row]
    is constant along a row and a gather from a wrong column is not."""
    rs = np.random.RandomState(8100)
    n = len(ATT_LENGTHS)
    ptr = np.concatenate([[0], np.cumsum(ATT_LENGTHS)]).astype(np.int32)
    e = int(ptr[-1])
    rows = np.repeat(np.arange(n), ATT_LENGTHS)
    half = rs.randint(0, ATT_COLS // 2, e)
    idx = (2 * half + rows % 2).astype(np.int32)
    el = np.where(np.arange(ATT_COLS) % 2 == 0, 1.0, 2.0).astype(np.float32)
    er = (np.arange(n) % 9 - 6).astype(np.float32)           # -6 .. 2: both leaky branches
    z = el[idx] + er[rows]
    logits = np.where(z > 0, z, z * np.float32(ATT_SLOPE)).astype(np.float32)
    alpha = (1.0 / np.repeat(np.maximum(ATT_LENGTHS, 1), ATT_LENGTHS)).astype(np.float32)
    ga = rs.randint(-4, 5, e).astype(np.float32)
    return types.SimpleNamespace(ptr=ptr, idx=idx, rows=rows, el=el, er=er, z=z, logits=logits,
                                 alpha=alpha, ga=ga, n=n, nc=ATT_COLS, e=e)


def attention_refs(c):
    """f64 (grad_logits, grad_edge, grad_er, grad_el) of attention_case from alpha and ga."""
    a, g = c.alpha.astype(np.float64), c.ga.astype(np.float64)
    dot = np.zeros(c.n, np.float64)
    np.add.at(dot, c.rows, a * g)
    gl = a * (g - dot[c.rows])
    ge = np.where(c.z > 0, gl, gl * ATT_SLOPE)
    ger = np.zeros(c.n, np.float64)
    np.add.at(ger, c.rows, ge)
    gel = np.zeros(c.nc, np.float64)
    np.add.at(gel, c.idx, ge)
    return gl, ge, ger, gel


# ---------------------------------------------------------------------------- the cases
Case = collections.namedtuple("Case", "id family target p")

BWD_SHAPES = {                      # (U, threads) -> the options that launch it
    (8, 1024): dict(),
    (12, 768): dict(bwd_waves=12, bwd_unroll=12),
    (8, 768): dict(bwd_waves=12, bwd_unroll=8),
    (16, 512): dict(bwd_waves=8, bwd_unroll=16),
    (12, 512): dict(bwd_waves=8, bwd_unroll=12),
    (8, 512): dict(bwd_waves=8, bwd_unroll=8),
}
FWD_FLAGS = {                       # (V, FL) -> (k, options) on the sweep's sparse graph
    (1, 0): (5, dict(fwd_chunk3=2)),
    (4, 0): (8, dict(fwd_chunk3=2)),
    (4, 1): (8, dict()),
    (4, 2): (32, dict()),
    (4, 3): (24, dict()),
    (4, 4): (16, dict(fwd_fixed=2)),
    (4, 6): (16, dict()),
}
FWD_SHAPES = {                      # (threads, sub-steps) -> options
    (256, 8): dict(fwd_waves=4),
    (512, 8): dict(fwd_waves=8, fwd_unroll=8),
    (512, 4): dict(fwd_waves=8, fwd_unroll=4),
}
FWD_ROWCONST_K = {2: 32, 3: 24, 6: 16}       # FL -> k on rowconst's tiles graph
PASS_CASES = [                      # statistics / pack pass: (target, k, options), sparse graph
    (_name("cbsr_stats4_kernel", 0, True), 32, dict()),
    (_name("cbsr_stats4_kernel", 1, True), 32, dict(fwd_two_tables=2)),
    (_name("cbsr_stats4_kernel", 1, False), 32, dict(fwd_two_tables=2, fwd_fixed=2)),
    (_name("cbsr_stats4_kernel", 2, True), 16, dict()),
    (_name("cbsr_stats4_kernel", 2, False), 16, dict(fwd_fixed=2)),
    (_name("pack_cbsr3_kernel", 3), 24, dict()),
    (_name("pack_cbsr3_kernel", 2), 18, dict(fwd_chunk3=3)),
]
TOPK_WIDTHS = {True: 256, False: 200}        # D == 256 or a partial row
TOPK_KS = {True: 72, False: 16}              # k > 64 or not
TOPK_VARIANTS = ["plain", "records", "dropout", "dense", "dense_dropout"]
SDDMM_KS = [3, 8, 13, 32, 64, 100, 256]      # 1, 2, 4, 8, 16, 32, 64 lanes per edge
DENSE_SPMM_DS = [16, 32, 64, 128, 256]


def _oid(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # forward: 7 (V, FL) x 3 shapes with 8-byte words, 3 FL x 2 shapes with 4-byte words
    for (v, fl), (k, o1) in FWD_FLAGS.items():
        for (nt, fu), o2 in FWD_SHAPES.items():
            opts = dict(o1, **o2)
            out.append(Case(f"fwd-V{v}-FL{fl}-{nt}x{fu}", "forward",
                            _name("spgemm_fwd_kernel", v, fl, nt, fu, False),
                            dict(graph="sparse", k=k, opts=opts)))
    for fl, k in FWD_ROWCONST_K.items():
        for waves, nt in ((4, 256), (8, 512)):
            out.append(Case(f"fwd-rowconst-FL{fl}-{nt}x8", "forward",
                            _name("spgemm_fwd_kernel", 4, fl, nt, 8, True),
                            dict(graph="tiles", k=k, opts=dict(fwd_waves=waves))))
    for target, k, opts in PASS_CASES:
        out.append(Case(f"pass-{target[len(NS):]}", "forward_pass", target,
                        dict(graph="sparse", k=k, opts=opts)))
    # column-block backward: 6 shapes x (F, Q), and the 4 of grad_out > 4 GiB
    for (u, nt), o1 in BWD_SHAPES.items():
        for (f, q), k in BIG_FQ.items():
            opts = dict(o1, bwd_algo=1, bwd_features_per_lane=f, bwd_slot_groups=1)
            out.append(Case(f"bwd-{u}x{nt}-F{f}-Q{int(q)}", "column_blocks",
                            _name("sspmm_bwd4_kernel", u, nt, f, q, False),
                            dict(graph="sparse", k=k, opts=opts)))
    for (f, q), k in BIG_FQ.items():
        opts = dict(bwd_algo=1, bwd_features_per_lane=f, bwd_slot_groups=1)
        out.append(Case(f"bwd-big-F{f}-Q{int(q)}", "bwd_big",
                        _name("sspmm_bwd4_kernel", 8, 512, f, q, True), dict(k=k, opts=opts)))
    for r, deg in TP_DEGREES.items():
        out.append(Case(f"rows-R{r}", "row_pass", _name("sspmm_bwd_rows_kernel", 4, r),
                        dict(deg=deg, opts=dict(bwd_algo=3))))
    # top-k: exact 2 x 2 x 2 x 5 (two dense pairs share a kernel) and the 8-row pair; ref 2 x 2 x 5
    for mode in sweep.MODES:
        for full, d in TOPK_WIDTHS.items():
            for wide, k in (TOPK_KS.items() if mode == "exact" else [(False, 16)]):
                for stats in (False, True):
                    for var in TOPK_VARIANTS:
                        kw = dict(stats=stats, records=var == "records",
                                  dropout=var in ("dropout", "dense_dropout"),
                                  dense=var.startswith("dense"))
                        out.append(Case(f"topk-{mode}-D{d}-k{k}-{'stats-' if stats else ''}{var}",
                                        "topk", topk_kernel(mode, 40, d, k, **kw),
                                        dict(mode=mode, n=40, d=d, k=k, **kw)))
    for full, d in TOPK_WIDTHS.items():
        out.append(Case(f"topk-exact-D{d}-k16-8rows", "topk",
                        _name("topk_exact_kernel", 8, False, full, False, False, False, False),
                        dict(mode="exact", n=TOPK_ROWS8, d=d, k=16, stats=False, records=False,
                             dropout=False, dense=False)))
    for drop in (False, True):
        for merge in (False, True):
            out.append(Case(f"scatter-drop{int(drop)}-merge{int(merge)}", "scatter",
                            scatter_kernel(drop, merge), dict(k=16, d=D, dropout=drop, merge=merge)))
    for k in SDDMM_KS:
        out.append(Case(f"sddmm-k{k}", "sddmm", sddmm_kernel(k), dict(k=k)))
    for d in DENSE_SPMM_DS:
        out.append(Case(f"dense-spmm-D{d}", "dense_spmm", dense_spmm_kernel(d), dict(d=d)))
    for name, (scenario, _, _) in SINGLES.items():
        out.append(Case(f"single-{name[len(NS):]}", "single", name, dict(scenario=scenario)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


# scenarios of the single-instance kernels that are plans: (graph, k, options)
PLAN_SCENARIOS = {
    "column_blocks": ("sparse", 16, dict(bwd_algo=1)),
    "row_order_2": ("sparse", 16, dict(bwd_algo=1, bwd_row_order=2)),
    "auto_row_order": ("dense", 16, dict(bwd_algo=1)),
    "scattered": ("sparse", 16, dict(bwd_algo=1, col_order="scattered")),
    "identity_order": ("sparse", 16, dict(bwd_algo=1)),
    "slab_flush": ("dense", 16, dict(bwd_algo=1, bwd_tasks_per_cu=64, bwd_min_task_edges=16)),
    "two_pass_chunks": ("sparse", 16, dict(bwd_algo=3, bwd_tp_chunks=2)),
    "split_rows": ("sparse", 5, dict(fwd_chunk3=2, fwd_task_cap=sweep.SPARSE_TASK_CAP)),
}
STATS_ODD_K = 18
REFRESH_K = 32                      # value_refresh: rowconst's tiles graph, default plan
