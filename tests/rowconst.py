"""Inputs of the row-constant forward tests (a plain module, no tests: tests/test_rowconst_inputs.py
checks what is built here on the CPU, tests/test_gpu_rowconst.py runs the kernels on it).

A plan keeps 4-byte forward edge words and one value per row when every edge of a destination
row carries the same value; `rowconst_rule` is that rule written once in numpy, and
`has_rowconst_kernel` says which default plans have a kernel of that form.
"""
import functools
import types

import numpy as np

import structured as st
from oracle import oracle

D = 256
TILE = 32                      # forward tile rows of a graph this small
VALUES = np.array([0.5, 1.0, 2.0], np.float32)


def rowconst_rule(ptr, val):
    """1 when the plan may sum a row with weight 1 and scale the sum once: in every row all edge
    values have the same bits, and that value is finite and not zero (0 * Inf and NaN terms must
    stay where the per-edge products put them). Rows of 0 or 1 edges pass. val None: all ones."""
    if val is None:
        return 1
    bits = np.ascontiguousarray(val, np.float32).view(np.uint32)
    for r in range(ptr.size - 1):
        b = bits[ptr[r]:ptr[r + 1]]
        if b.size == 0:
            continue
        if (b != b[0]).any() or (b[0] & 0x7fffffff) == 0 or (b[0] & 0x7f800000) == 0x7f800000:
            return 0
    return 1


def has_rowconst_kernel(k, fwd_fixed=True):
    """Whether the default plan of this k runs a forward kernel with a 4-byte form: fixed point
    (default from k = 16), quad-shared windows, i.e. the lanes of an edge (k / 2 pair chunks at
    k = 16, ceil(k / 3) lane chunks when k % 16 != 0, else k / 4) a multiple of 4, and 8 sub-steps
    (not k = 48)."""
    if not fwd_fixed or k < 16 or k == 48:
        return False
    lanes = k // 2 if k == 16 else (k + 2) // 3 if k % 16 else k // 4
    return lanes % 4 == 0


def oracle_forward(ptr, idx, val, data, sel):
    """(ref, mag) [rows, D] of a rectangular graph: the oracle takes a square one, so ptr is
    padded with edgeless rows up to the table's row count and the result cut back."""
    n, nc = ptr.size - 1, data.shape[0]
    assert n <= nc
    full = np.concatenate([ptr, np.full(nc - n, ptr[-1], ptr.dtype)])
    ref, mag = oracle.spgemm_forward(full, idx, val, data, sel, D, with_mag=True)
    return ref[:n], mag[:n]


def row_values(ptr, per_row):
    """Edge values [E]: row r's edges all carry per_row[r]."""
    return np.repeat(np.asarray(per_row, np.float32), np.diff(ptr)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tiles_graph():
    """(ptr, idx): 130 rows x 500 columns, four whole 32-row tiles and a partial one of 2 rows;
    tile 2 (rows 64..95) has no edge, row 0 has none, row 1 one, row 129 (the partial tile) one;
    the others 2..60, columns sorted within a row, repeats allowed."""
    rs = np.random.RandomState(130)
    n, nc = 130, 500
    deg = rs.randint(2, 61, n)
    deg[64:96] = 0
    deg[0], deg[1], deg[129] = 0, 1, 1
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.concatenate([np.sort(rs.randint(0, nc, d)) for d in deg]).astype(np.int32)
    return ptr.astype(np.int32), idx


@functools.lru_cache(maxsize=None)
def heavy_graph():
    """(ptr, idx): 40 rows x 500 columns; row 3 has 9,000 edges with repeated columns (above
    the forward's task cap: split into segments, summed atomically), the others 1..40."""
    rs = np.random.RandomState(9000)
    n, nc = 40, 500
    deg = rs.randint(1, 41, n)
    deg[3] = 9000
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.concatenate([np.sort(rs.randint(0, nc, d)) for d in deg]).astype(np.int32)
    return ptr.astype(np.int32), idx


GRAPHS = {"tiles": tiles_graph, "heavy": heavy_graph}
NCOLS = 500


@functools.lru_cache(maxsize=None)
def exact_case(gname, k, values_seed=1, dup=False, break_row=None):
    """Integer features, per-row values from {0.5, 1, 2}: exactly summable, so the kernels must
    equal the f64 oracle as floats. dup: half of the table rows repeat their first selector in
    slots 0 and 1 (repeated selectors are summed). break_row: one edge of that row takes another
    of the three values (no longer row-constant)."""
    p, ix = GRAPHS[gname]()
    n = p.size - 1
    rs = np.random.RandomState(values_seed)
    v = row_values(p, rs.choice(VALUES, n))
    if break_row is not None:
        e = int(p[break_row]) + 1
        assert p[break_row + 1] - p[break_row] >= 2
        v[e] = 0.5 if v[e] != 0.5 else 2.0
    x = st.int_features(NCOLS, D, seed=3000 + k)
    od, oi = oracle.maxk(x, k)
    if dup:
        oi = oi.copy()
        oi[::2, 1] = oi[::2, 0]
    ref, mag = oracle_forward(p, ix, v, od, oi)
    return types.SimpleNamespace(p=p, ix=ix, v=v, n=n, k=k, od=od, oi=oi, x=x, ref=ref, mag=mag)


# ---------------------------------------------------------------------------- wide range
RANGE_E = 20


@functools.lru_cache(maxsize=None)
def range_case():
    """Fixed-point and f64 tasks in one launch, with row-constant values: the tables of
    structured.range_tables (256 columns, k = 16, |x| in [1, 2)) with the odd columns scaled by
    2^-20 (structured's `columns` case: the call's statistic is max |x| < 2^1, min |x| >= 2^-20),
    on 96 rows: tiles 0 and 2 have 8 edges per row, tile 1 has 128. With unit weights a task's
    bound is its largest row's edge count, so the 8-edge tiles keep fixed point and the 128-edge
    tile exceeds the 2^-25 budget and sums in f64 (`fixed_tasks` replays the rule)."""
    rs = np.random.RandomState(96)
    data, sel = st.range_tables()
    data = data.copy()
    data[1::2] *= np.float32(2.0 ** -RANGE_E)
    n, nc = 96, st.RANGE_N
    deg = np.full(n, 8)
    deg[32:64] = 128
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.concatenate([np.sort(rs.randint(0, nc, d)) for d in deg]).astype(np.int32)
    ptr = ptr.astype(np.int32)
    v = row_values(ptr, rs.uniform(1.0, 2.0, n) * rs.choice([-1.0, 1.0], n))
    ref, mag = oracle_forward(ptr, idx, v, data, sel)
    return types.SimpleNamespace(p=ptr, ix=idx, v=v, n=n, k=st.RANGE_K, od=data, oi=sel, ref=ref,
                                 mag=mag)


def fixed_tasks(ptr, data, tile=TILE):
    """The per-task fixed-point decision for unit weights (spgemm.hip, fwd_fix_scale; plan.hip,
    fwd_fix_stats_kernel) on tables with distinct selectors: task t is fixed point iff
    gexp + ex - en <= 25, with 2^ex > max |x|, 2^en <= min nonzero |x|, and gexp = es where
    (largest row's edge count) * (1 + 2^-10) < 2^es (every |val| is 1 = 2^0)."""
    a = np.abs(data[data != 0]).astype(np.float64)
    ex = int(np.floor(np.log2(a.max()))) + 1
    en = int(np.floor(np.log2(a.min())))
    deg = np.diff(ptr)
    out = []
    for r0 in range(0, deg.size, tile):
        s = float(np.float32(deg[r0:r0 + tile].max()) * np.float32(1.0 + 2.0 ** -10))
        if s == 0:
            out.append(True)          # an edgeless task adds nothing either way
            continue
        es = int(np.frexp(s)[1])
        out.append(es + ex - en <= 25)
    return out


# ---------------------------------------------------------------------------- non-finite
@functools.lru_cache(maxsize=None)
def nonfinite_case(k, kind):
    """tiles graph, N(0, 1)-like features, per-row values of magnitude in [0.5, 1):

    val_nan / val_inf: row 10 (row 40) carries NaN (+Inf, row 41 -Inf) on every edge: still the
                       same bits along the row, but the plan must keep the 8-byte words;
    table:             finite row-constant values, +Inf, -Inf and NaN entries in table rows that
                       have in-edges, and a zero entry beside an Inf one (the 4-byte form: the row
                       sums carry them, the one scaling keeps sign and NaN)."""
    p, ix = tiles_graph()
    n = p.size - 1
    rs = np.random.RandomState(77 + k)
    per_row = (rs.uniform(0.5, 1.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    x = rs.randn(NCOLS, D).astype(np.float32)
    od, oi = oracle.maxk(x, k)
    od = od.copy()
    if kind == "val_nan":
        per_row[10] = np.nan
    elif kind == "val_inf":
        per_row[40], per_row[41] = np.inf, -np.inf
    else:
        assert kind == "table", kind
        c = [int(ix[p[r]]) for r in (10, 40, 100)]
        assert len(set(c)) == 3
        od[c[0], 3], od[c[0], 4] = np.inf, 0.0
        od[c[1], 0] = -np.inf
        od[c[2], k - 1] = np.nan
    v = row_values(p, per_row)
    ref, mag = oracle_forward(p, ix, v, od, oi)
    return types.SimpleNamespace(p=p, ix=ix, v=v, n=n, k=k, od=od, oi=oi, ref=ref, mag=mag)
