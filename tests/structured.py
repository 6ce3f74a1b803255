"""Structured parity inputs: hub-column graphs, exactly summable data, wide value ranges and
non-finite values, with the comparison helpers their tests share (a plain module, no tests:
tests/test_structured_inputs.py checks what is built here on the CPU,
tests/test_gpu_structured.py runs the kernels on it).

Every other parity input of the suite is N(0, 1) features on graphs without a hub column and
benign edge values; these inputs are chosen so that one lost, doubled or misplaced update, a
wrong per-task fixed-point decision or a hidden NaN changes a checked number.
"""
import functools
import itertools
import types

import numpy as np

from maxk_kernels import graphs
from oracle import oracle
from test_dropout_capi import drop_scale, dropped_table, keep_mask
from test_gpu_parity import GRAPHS

U24 = 2.0 ** -24                       # unit roundoff of f32
FWD_REL = 2.0 ** -24 + 2.0 ** -23      # the fixed-point / f64 forward's bound (test_gpu_parity)
EXACT_LIMIT = 2.0 ** 22                # sum |terms| up to which multiples of 0.5 add exactly
RTOL = 1e-5


# ---------------------------------------------------------------------------- graphs
def star(n):
    """(ptr, idx) int32: every row r has edges to the columns {0, 1, n - 1, r}; rows 0, 1 and
    n - 1 have edges to every column. Columns are sorted and unique per row. The hub columns
    0, 1 and n - 1 have in-degree n, every other column 4 (its own row and the three hub rows);
    E = 7 n - 12. Columns 0 and 1 are neighbours, column n - 1 is the last one."""
    assert n >= 4
    hubs = (0, 1, n - 1)
    deg = np.full(n, 4, np.int64)
    deg[list(hubs)] = n
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.empty(ptr[-1], np.int32)
    full = np.arange(n, dtype=np.int32)
    for h in hubs:
        idx[ptr[h]:ptr[h + 1]] = full
    r = np.arange(2, n - 1, dtype=np.int64)
    base = ptr[r]
    idx[base] = 0
    idx[base + 1] = 1
    idx[base + 2] = r
    idx[base + 3] = n - 1
    return ptr.astype(np.int32), idx


def all_to_one(n):
    """(ptr, idx) int32: one edge per row, all to column 0 (a star with one centre): column 0
    has in-degree n, and every lane of every wave of the backward updates the same slots."""
    return np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32)


def col_degrees(ptr, idx):
    """In-degree of every column of a square CSR."""
    return np.bincount(idx, minlength=ptr.size - 1)


# ---------------------------------------------------------------------------- A: exact
EXACT_GRAPHS = {
    # E = 7 n - 12 = 139,988 (the star's definition; above the 130,000 the other cases keep to)
    "star20000": lambda: star(20_000),
    "all_to_one4097": lambda: all_to_one(4097),
    "synthetic": lambda: GRAPHS["synthetic"]()[:2],
}
EXACT_DK = [(256, 16), (256, 8), (256, 32), (256, 64), (256, 7), (100, 10)]
EXACT_SEED = 0x5EEDF00D12345678
EXACT_VALUE_SEEDS = {"star20000": 9, "all_to_one4097": 14, "synthetic": 9}   # of the edge values


@functools.lru_cache(maxsize=4)
def int_features(n, d, seed):
    """f32 [n, d], integer-valued in [-4, 4] (round(2 N(0, 1)), clipped), no -0.0. Cached and
    shared: read only."""
    rs = np.random.RandomState(seed)
    return (np.clip(np.round(rs.randn(n, d) * 2.0), -4.0, 4.0) + 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_graph(gname):
    """(ptr, idx, val) of an EXACT_GRAPHS entry with edge values drawn from {0.5, 1, 2}."""
    p, ix = EXACT_GRAPHS[gname]()
    rs = np.random.RandomState(EXACT_VALUE_SEEDS[gname])
    v = rs.choice(np.array([0.5, 1.0, 2.0], np.float32), ix.size).astype(np.float32)
    return p, ix, v


def exactly_summable(*mags):
    """The exactness precondition: every term is a multiple of 0.5 (integer features times
    values in {0.5, 1, 2}, dropout scale 2), so while an output's sum of |terms| stays
    <= 2^22 every partial sum, in any order, is a multiple of 0.5 below 2^23 and exact in
    f32 (and in f64, and in the fixed-point residues). True when every `mag` array is finite
    and within that limit."""
    return all(np.isfinite(m).all() and float(np.max(m, initial=0.0)) <= EXACT_LIMIT
               for m in mags)


@functools.lru_cache(maxsize=2)
def exact_case(gname, d, k, mode="exact", dropout_p=0.0):
    """Inputs and f64-oracle results of one exact-arithmetic case: integer features x and
    gradient g, the top-k table (through the numpy dropout mask when dropout_p > 0), forward,
    backward and input-gradient references with their magnitudes."""
    p, ix, v = exact_graph(gname)
    n = p.size - 1
    x = int_features(n, d, seed=1000 + k)
    g = int_features(n, d, seed=2000 + k)
    od0, oi = oracle.maxk(x, k, mode)
    od = dropped_table(od0, oi, dropout_p, EXACT_SEED) if dropout_p else od0
    fwd, fwd_mag = oracle.spgemm_forward(p, ix, v, od, oi, d, with_mag=True)
    bwd, bwd_mag = oracle.sspmm_backward(p, ix, v, g, oi, with_mag=True)
    # x.grad of maxk_aggregate: the filled slots' gradients (times the kept mask and scale)
    # scattered to their features; ref_compat padding slots (0.0f at selector 0) carry none
    filled = od0 != 0 if mode == "ref_compat" else np.ones_like(od0, bool)
    scale = float(drop_scale(dropout_p)) if dropout_p else 1.0
    keep = keep_mask(dropout_p, EXACT_SEED, np.arange(n)[:, None], oi) if dropout_p else 1.0
    rows = np.repeat(np.arange(n)[:, None], k, 1)
    gx = np.zeros((n, d), np.float64)
    gx_mag = np.zeros((n, d), np.float64)
    gx[rows[filled], oi[filled]] = (bwd.astype(np.float64) * keep * scale)[filled]
    gx_mag[rows[filled], oi[filled]] = (bwd_mag.astype(np.float64) * scale)[filled]
    return types.SimpleNamespace(p=p, ix=ix, v=v, n=n, d=d, k=k, x=x, g=g, od0=od0, od=od,
                                 oi=oi, fwd=fwd, fwd_mag=fwd_mag, bwd=bwd, bwd_mag=bwd_mag,
                                 gx=gx, gx_mag=gx_mag)


# ---------------------------------------------------------------------------- B: hub sums
HUB_CASES = {
    # name: (star size = hub in-degree, grad_out, edge values)
    "n4096_random": (4096, "absnormal", "uniform"),
    "n16385_random": (16385, "absnormal", "uniform"),
    "n16385_g0.1_v1": (16385, 0.1, 1.0),
    "n16385_g1_v1/37": (16385, 1.0, 1.0 / 37.0),
}
HUB_D, HUB_K = 256, 16


@functools.lru_cache(maxsize=2)
def hub_case(name):
    """A star graph with same-sign terms: g = |N(0, 1)| or a constant, val = U(0.5, 1) or a
    constant; selectors of N(0, 1) features; the forward's table carries g's first k columns
    (same-sign terms on the hub rows too). f64-oracle results of both directions."""
    n, gk, vk = HUB_CASES[name]
    p, ix = star(n)
    rs = np.random.RandomState(n)
    g = (np.abs(rs.randn(n, HUB_D)) if gk == "absnormal"
         else np.full((n, HUB_D), gk)).astype(np.float32)
    v = (rs.uniform(0.5, 1.0, ix.size) if vk == "uniform"
         else np.full(ix.size, vk)).astype(np.float32)
    _, oi = oracle.maxk(graphs.features(n, HUB_D, seed=n).numpy(), HUB_K)
    od = np.ascontiguousarray(g[:, :HUB_K])
    bwd, bwd_mag = oracle.sspmm_backward(p, ix, v, g, oi, with_mag=True)
    fwd, fwd_mag = oracle.spgemm_forward(p, ix, v, od, oi, HUB_D, with_mag=True)
    return types.SimpleNamespace(p=p, ix=ix, v=v, n=n, g=g, od=od, oi=oi, bwd=bwd,
                                 bwd_mag=bwd_mag, fwd=fwd, fwd_mag=fwd_mag,
                                 ncol=col_degrees(p, ix))


FWD_TASK_CAP = 4096     # the forward's default task cap: longer rows are split into segments


def split_row_segments(c, r, rounded_products):
    """f32 sums [S, D] of the forward's segments of row r of a hub case: its edges in CSR
    order, FWD_TASK_CAP at a time (16,385 edges: 4 x 4096 and 1), each segment summed in f64
    and rounded once, as both forward paths do (the f64 path rounds every product to f32
    first: `rounded_products`; the fixed-point path adds the exact products)."""
    e0, e1 = int(c.p[r]), int(c.p[r + 1])
    segs = []
    for a in range(e0, e1, FWD_TASK_CAP):
        b = min(a + FWD_TASK_CAP, e1)
        cols = c.ix[a:b]
        t = c.v[a:b, None] * c.od[cols] if rounded_products else \
            c.v[a:b, None].astype(np.float64) * c.od[cols]
        acc = np.zeros(HUB_D)
        np.add.at(acc, c.oi[cols].astype(np.int64), t.astype(np.float64))
        segs.append(acc.astype(np.float32))
    return np.array(segs)


def worst_segment_order(c, r, rounded_products):
    """A split row's segments are added into the zeroed output row with f32 atomics, in any
    order: the largest |sum - ref| / |ref| against the f32 oracle row over every order of the
    adds (S! of them) and every feature, as oracle.worst_relative measures it."""
    segs = split_row_segments(c, r, rounded_products)
    ref = c.fwd[r].astype(np.float64)
    worst = 0.0
    for order in itertools.permutations(range(len(segs))):
        a = np.zeros(HUB_D, np.float32)
        for i in order:
            a = a + segs[i]                  # f32 + f32 -> f32, rounded to nearest
        worst = max(worst, float((np.abs(a.astype(np.float64) - ref) / np.abs(ref)).max()))
    return worst, len(segs)


def split_row_bound(segments):
    """(S + 2) 2^-24 relative, what a same-sign row split into S segments owes: the products'
    rounding (f64 path), the S segment sums' rounding, S - 1 f32 additions, the rounding of
    the f32 reference."""
    return (segments + 2) * U24


def summation_bound(ncol, mag):
    """(n_c + 2) 2^-24 mag per element of grad_sp [N, k]: n_c f32 products (one rounding each)
    added in any order (n_c - 1 roundings), plus the rounding of the f32 reference; n_c is the
    column's in-degree, from the CSR."""
    return (np.asarray(ncol, np.float64)[:, None] + 2.0) * U24 * np.asarray(mag, np.float64)


def running_sum_model(c, col):
    """Sequential f32 sum (numpy cumsum in float32) of the f32 products val * g[r, f] of column
    `col`'s in-edges, in row order, per selector slot: (model [k] f32, the f64 sum [k])."""
    rows = np.repeat(np.arange(c.n), np.diff(c.p))
    e = np.flatnonzero(c.ix == col)
    terms = (c.v[e, None] * c.g[rows[e]][:, c.oi[col]]).astype(np.float32)     # [n_c, k]
    model = np.cumsum(terms, axis=0, dtype=np.float32)[-1]
    return model, terms.astype(np.float64).sum(axis=0)


# ---------------------------------------------------------------------------- C: ranges
RANGE_N, RANGE_D, RANGE_K, RANGE_TILE = 256, 256, 16, 32
RANGE_E = [0, 8, 16, 20, 22, 24, 26, 30, 40, 60, 100]
MIN_PRODUCT = 2.0 ** -100


@functools.lru_cache(maxsize=None)
def range_graph():
    """(ptr, idx, special) for the range tests: 256 rows of 8 edges; 7 sources of a row lie in
    the residue classes 1..15 mod 16 and one, the `special` edge (a bool mask over the edges),
    in class 0. With `range_tables` a source c selects the features [16 (c mod 16), +16), so
    the features 0..15 of a row receive the special edge's terms and nothing else."""
    rs = np.random.RandomState(77)
    n = RANGE_N
    regular = np.flatnonzero(np.arange(n) % 16 != 0)
    zero_class = np.flatnonzero(np.arange(n) % 16 == 0)
    idx = np.empty((n, 8), np.int32)
    for r in range(n):
        idx[r, :7] = rs.choice(regular, 7, replace=False)
        idx[r, 7] = rs.choice(zero_class)
    idx.sort(axis=1)
    ptr = (np.arange(n + 1) * 8).astype(np.int32)
    idx = idx.reshape(-1)
    return ptr, idx, idx % 16 == 0


@functools.lru_cache(maxsize=None)
def range_tables():
    """(sp_data, sp_index) [256, 16]: source c selects the features 16 (c mod 16) + 0..15,
    with values of magnitude in [1, 2) and random signs."""
    rs = np.random.RandomState(78)
    n, k = RANGE_N, RANGE_K
    sel = (16 * (np.arange(n) % 16))[:, None] + np.arange(k)[None, :]
    data = rs.uniform(1.0, 2.0, (n, k)) * rs.choice([-1.0, 1.0], (n, k))
    return data.astype(np.float32), sel.astype(np.uint8)


def range_values(case, e=0):
    """(val, sp_data) of one range case on `range_graph`; |val| in [1, 2) before scaling.

    rows:    the odd rows of every 32-row tile carry values 2^-e times the even rows';
    within:  the special edge of every row is scaled by 2^-e;
    mixed:   tile 0 is benign, the odd rows of tile 1 (rows 32..63) are scaled by 2^-60;
    zeros:   the `rows` values, with every 5th edge value exactly 0, row 5 all zero and tile 3
             (rows 96..127) all zero;
    columns: the table rows of the odd source columns are scaled by 2^-e (the call's global
             statistic); the edge values stay benign.
    """
    ptr, idx, special = range_graph()
    data, _ = range_tables()
    rs = np.random.RandomState(79)
    val = rs.uniform(1.0, 2.0, idx.size) * rs.choice([-1.0, 1.0], idx.size)
    rows = np.repeat(np.arange(RANGE_N), np.diff(ptr))
    s = 2.0 ** -e
    if case in ("rows", "zeros"):
        val[rows % 2 == 1] *= s
    elif case == "within":
        val[special] *= s
    elif case == "mixed":
        val[(rows % 2 == 1) & (rows // RANGE_TILE == 1)] *= 2.0 ** -60
    elif case == "columns":
        data = data.copy()
        data[1::2] *= np.float32(s)
    else:
        assert case == "benign", case
    if case == "zeros":
        val[::5] = 0.0
        val[rows == 5] = 0.0
        val[rows // RANGE_TILE == 3] = 0.0
    return val.astype(np.float32), data


def products_normal(ptr, idx, val, data):
    """C's precondition: every nonzero product |val x| of the forward is a normal f32 of at
    least 2^-100 (the f64 path rounds the product in f32) and no row's sum of |products| gets
    near overflow. Returns (smallest nonzero |product|, largest row sum)."""
    a = np.abs(val.astype(np.float64))
    xmin = np.where(data != 0, np.abs(data.astype(np.float64)), np.inf).min(axis=1)
    xmax = np.abs(data.astype(np.float64)).max(axis=1)
    lo = np.where(a > 0, a * xmin[idx], np.inf).min()
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    hi = np.bincount(rows, weights=a * xmax[idx]).max()
    return float(lo), float(hi)


# ---------------------------------------------------------------------------- D: non-finite
NONFINITE_FWD = ["val", "table_inf", "table_nan", "padding_times_inf", "zero_times_inf"]
NONFINITE_BWD = ["val", "g_nan_f0", "g_inf_f0", "g_nan_selected", "g_inf_selected",
                 "g_nan_unselected", "g_inf_unselected", "zero_times_inf"]
NONFINITE_D = 256


def nonfinite_case(k, case):
    """synthetic_csr(300, 3000) with N(0, 1) features and gradient, exact top-k tables and
    values +-U(0.5, 1), and one kind of non-finite input (the fields are the arrays to run):

    val:               NaN, +Inf and -Inf each on one edge value, in the rows 10, 100 and 200;
    table_inf / _nan:  +Inf and -Inf (NaN) entries in sp_data rows that have in-edges;
    padding_times_inf: an Inf-valued edge whose source column's table ends in ref_compat padding
                       slots (0.0f at selector 0): 0 * Inf = NaN at feature 0 of the edge's row;
    zero_times_inf:    a zero edge value whose source's table (forward) / whose row of grad_out
                       (backward) holds an Inf at a feature the edge reads: NaN;
    g_*_f0 / _selected / _unselected: grad_out[r, f] = NaN or Inf at f = 0 (which the backward's
                       padding slots gather), at a feature a neighbour of r selects, and at one
                       none of them selects (`unselected`: the reference stays finite).
    """
    pt, it = graphs.synthetic_csr(300, 3000, seed=61)
    p, ix = pt.numpy(), it.numpy()
    n, d = p.size - 1, NONFINITE_D
    rs = np.random.RandomState(62)
    v = (rs.uniform(0.5, 1.0, ix.size) * rs.choice([-1.0, 1.0], ix.size)).astype(np.float32)
    g = graphs.features(n, d, seed=63).numpy().copy()
    od, oi = oracle.maxk(graphs.features(n, d, seed=64).numpy(), k)
    od, oi = od.copy(), oi.copy()
    assert (np.diff(p)[[10, 100, 200, 50]] >= 2).all()
    r = 50                                   # the row the single-edge cases use
    e = int(p[r])                            # its first edge
    c = int(ix[e])
    if case == "val":
        v[p[10]], v[p[100] + 1], v[p[200]] = np.nan, np.inf, -np.inf
    elif case == "table_inf":
        od[ix[p[10]], 3], od[ix[p[100]], 5] = np.inf, -np.inf
    elif case == "table_nan":
        od[ix[p[10]], 0], od[ix[p[100]], k - 1] = np.nan, np.nan
    elif case == "padding_times_inf":
        v[e] = np.inf
        od[c, k // 2:], oi[c, k // 2:] = 0.0, 0
    elif case == "zero_times_inf":
        v[e] = 0.0
        od[c, 2] = np.inf                    # forward: 0 * Inf at out[r, oi[c, 2]]
        g[r, oi[c, 2]] = np.inf              # backward: 0 * Inf at grad_sp[c, 2]
    else:
        kind, where = case.split("_")[1:]
        if where == "f0":                    # a row with a neighbour that selects feature 0
            r = next(i for i in range(n) if (oi[ix[p[i]:p[i + 1]]] == 0).any())
            c = int(ix[p[r]])
        chosen = set(oi[ix[p[r]:p[r + 1]]].reshape(-1).tolist())
        if where == "f0":
            f = 0
        elif where == "selected":
            f = int(oi[c, min(3, k - 1)])
        else:
            f = next(f for f in range(1, d) if f not in chosen)
        if where != "f0":
            assert (f in chosen) == (where == "selected")
        g[r, f] = np.nan if kind == "nan" else np.inf
    fwd, fwd_mag = oracle.spgemm_forward(p, ix, v, od, oi, d, with_mag=True)
    bwd, bwd_mag = oracle.sspmm_backward(p, ix, v, g, oi, with_mag=True)
    return types.SimpleNamespace(p=p, ix=ix, v=v, n=n, d=d, k=k, g=g, od=od, oi=oi, fwd=fwd,
                                 fwd_mag=fwd_mag, bwd=bwd, bwd_mag=bwd_mag, r=r)


def assert_same_nonfinite_and_close(got, ref, mag, rtol=RTOL):
    """The oracle's IEEE f64 sums are the specification of non-finite data: `got` has its NaNs
    exactly where `ref` has them, its +Inf and -Inf exactly where `ref` has them (with the
    sign), and every element whose reference is finite is within the fp32-accumulator bar
    (oracle.close_enough). Returns the worst err / bound over the finite elements."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    mag = np.asarray(mag, np.float64)
    assert got.shape == ref.shape == mag.shape

    def where(m):
        return [tuple(int(i) for i in t) for t in np.argwhere(m)[:8]]

    hidden = np.isnan(ref) & ~np.isnan(got)
    assert not hidden.any(), f"NaN of the reference missing at {where(hidden)}: {got[hidden][:8]}"
    spread = np.isnan(got) & ~np.isnan(ref)
    assert not spread.any(), f"NaN where the reference has {ref[spread][:8]} at {where(spread)}"
    for s, name in ((np.inf, "+Inf"), (-np.inf, "-Inf")):
        bad = (ref == s) != (got == s)
        assert not bad.any(), (f"{name} positions differ at {where(bad)}: got {got[bad][:8]}, "
                               f"reference {ref[bad][:8]}")
    fin = np.isfinite(ref)
    assert np.isfinite(mag[fin]).all(), "a finite reference with a non-finite magnitude"
    ok, worst = oracle.close_enough(got[fin], ref[fin], mag[fin], rtol=rtol)
    assert ok, f"finite elements: worst err/bound = {worst:.3g}"
    return worst
