"""Shared by tests/test_gat_heads_capi.py (CPU) and tests/test_gpu_gat_heads.py (GPU): the test
graph, the float64 restatements of the three multi-head formulas of include/maxk_hip.h
("Multi-head aggregation"), their derived bounds, and the restated selectors of
csrc/variants_heads.h.

Everything is numpy on the host. alpha is head-major [H, E]; F = D // H; the head of feature s is
s // F. Products of two f32 values are exact in float64 (48 significant bits), so the float64
sums below differ from the exact ones by float64 rounding only."""
import functools

import numpy as np

U = 2.0 ** -24
LIMITS = (16, 512, 16, 512)     # maxk_heads_row_limits, asserted against the library by the tests
NUM = 600                        # rows and columns of the test graph
# (D, H, k) of the issue's table, and one more for the remaining backward instantiation
SHAPES = ((256, 8, 16), (256, 4, 32), (64, 2, 8), (96, 3, 10), (256, 16, 64), (256, 2, 100),
          (256, 1, 16), (256, 8, 32))


# ------------------------------------------------------------------ selectors, restated
def heads_lanes(k):
    lp = 8
    while lp < k and lp < 64:
        lp *= 2
    return lp


def fwd_kernel_name(k):
    return f"maxk_mh::heads_fwd_kernel<{heads_lanes(k)}>"


def bwd_kernel_name(k, num_heads):
    hp = 4 if num_heads <= 4 else 16
    return f"maxk_mh::heads_bwd_kernel<{max(heads_lanes(k), hp)}, {hp}>"


# the head-batched attention kernels (csrc/gat_attention.hip): one instantiation each
ATTENTION_KERNELS = ("maxk_mh::gat_attention_fwd_heads_kernel",
                     "maxk_mh::gat_attention_bwd_heads_kernel",
                     "maxk_mh::edge_colsum_heads_kernel")


def regime(n, limits=LIMITS[:2]):
    """0, 1 or 2: the regime that serves a row (column) of n edges."""
    return 0 if n <= limits[0] else 1 if n <= limits[1] else 2


# ------------------------------------------------------------------ graphs
DESIGNED = (0, 0, 1, 2, LIMITS[0] - 1, LIMITS[0], LIMITS[0] + 1, LIMITS[1] - 1, LIMITS[1],
            LIMITS[1] + 1, 100)
HUB_ROW, HUB_COL = 5000, 3000
ND = len(DESIGNED) + 1          # designed rows 0 .. ND-1, designed columns 0 .. ND-1


def csr_from_edges(rows, cols, num_rows):
    """CSR of the edges in their given order within each row (stable)."""
    order = np.argsort(rows, kind="stable")
    ptr = np.zeros(num_rows + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=num_rows), out=ptr[1:])
    return ptr.astype(np.int32), cols[order].astype(np.int32)


@functools.lru_cache(maxsize=None)
def graph_arrays():
    """(ptr, idx) int32 of the 600 x 600 test graph. Rows 0 .. ND-1 have exactly the designed
    lengths (0, 1, 2, each limit - 1 / at / + 1, 100 and the hub row of 5,000 edges) and take
    their columns from the undesigned ones; columns 0 .. ND-1 have exactly the designed lengths
    (hub column: 3,000) and take their rows from the undesigned ones; the rest is random, short
    and medium. The hubs repeat (row, column) pairs by construction."""
    rng = np.random.default_rng(15)
    rows, cols = [], []
    for r, n in enumerate(DESIGNED + (HUB_ROW,)):
        rows.append(np.full(n, r))
        cols.append(rng.integers(ND, NUM, n))
    for c, n in enumerate(DESIGNED + (HUB_COL,)):
        rows.append(rng.integers(ND, NUM, n))
        cols.append(np.full(n, c))
    deg = rng.integers(0, 30, NUM - ND)
    for r, n in enumerate(deg, start=ND):
        rows.append(np.full(n, r))
        cols.append(rng.integers(ND, NUM, n))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    perm = rng.permutation(rows.size)
    ptr, idx = csr_from_edges(rows[perm], cols[perm], NUM)
    rlen, clen = np.diff(ptr), np.bincount(idx, minlength=NUM)
    want = DESIGNED + (HUB_ROW,)
    assert tuple(rlen[:ND]) == want and tuple(clen[:ND]) == DESIGNED + (HUB_COL,)
    key = rows_of(ptr).astype(np.int64) * NUM + idx
    assert np.unique(key).size < key.size          # repeated (row, column) pairs
    assert {regime(int(n)) for n in rlen} == {0, 1, 2} == {regime(int(n)) for n in clen}
    for a in (ptr, idx):
        a.setflags(write=False)
    return ptr, idx


def rows_of(ptr):
    return np.repeat(np.arange(ptr.size - 1), np.diff(ptr))


def transposed(ptr, idx, num_cols):
    """(ptr_t, idx_t, order) int32: the transposed structure as CSRGraph builds it (entries of a
    column by ascending row, ties in CSR order)."""
    rows = rows_of(ptr)
    order = np.argsort(idx.astype(np.int64) * (ptr.size - 1) + rows, kind="stable")
    ptr_t = np.zeros(num_cols + 1, np.int64)
    np.cumsum(np.bincount(idx, minlength=num_cols), out=ptr_t[1:])
    return ptr_t.astype(np.int32), rows[order].astype(np.int32), order.astype(np.int32)


# One tile of 16 rows holds two adjacent hubs, a medium, a short and an empty row; the next is all
# short; row 32 is alone in the last tile (15 positions past num_rows), medium at exactly the limit.
TILE_ROWS, TILE_COLS = 33, 700
TILE_LENGTHS = {0: 600, 1: LIMITS[1] + 1, 2: LIMITS[0] + 1, 3: LIMITS[0], 4: 0, 32: LIMITS[1]}


@functools.lru_cache(maxsize=None)
def tile_graph():
    """(ptr, idx) int32 of the 33 x 700 graph above; rows 5 .. 31 are short, of random length."""
    rng = np.random.default_rng(33)
    lengths = rng.integers(0, LIMITS[0] + 1, TILE_ROWS)
    for r, n in TILE_LENGTHS.items():
        lengths[r] = n
    rows = np.repeat(np.arange(TILE_ROWS), lengths)
    ptr, idx = csr_from_edges(rows, rng.integers(0, TILE_COLS, rows.size), TILE_ROWS)
    want = [2, 2, 1, 0, 0] + [0] * 27 + [1]
    assert [regime(int(n)) for n in np.diff(ptr)] == want
    for a in (ptr, idx):
        a.setflags(write=False)
    return ptr, idx


@functools.lru_cache(maxsize=None)
def tile_graph_t():
    """(ptr, idx) of the 700 x 33 graph whose columns have tile_graph's row lengths, for the
    backward's walk over columns; its rows are short."""
    ptr, idx = tile_graph()
    tp, ti = csr_from_edges(idx.astype(np.int64), rows_of(ptr), TILE_COLS)
    assert np.array_equal(np.bincount(ti, minlength=TILE_ROWS), np.diff(ptr))
    for a in (tp, ti):
        a.setflags(write=False)
    return tp, ti


@functools.lru_cache(maxsize=None)
def short_graph(n):
    """(ptr, idx) of an n x n graph whose rows and columns are all short: row 0 and every fourth
    row after it at exactly the short limit (or n, if that is less), some rows empty."""
    rng = np.random.default_rng(100 + n)
    top = min(n, LIMITS[0])
    lengths = rng.integers(0, min(n, 6) + 1, n)
    lengths[::4] = top
    rows = np.repeat(np.arange(n), lengths)
    ptr, idx = csr_from_edges(rows, rng.integers(0, n, rows.size), n)
    rlen, clen = np.diff(ptr), np.bincount(idx, minlength=n)
    assert max(rlen.max(), clen.max()) <= LIMITS[0] and (rlen == top).sum() >= (n + 3) // 4
    assert n == 1 or (rlen == 0).any()
    for a in (ptr, idx):
        a.setflags(write=False)
    return ptr, idx


def small_graph(n=40, seed=2):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 9, n)
    rows = np.repeat(np.arange(n), deg)
    return csr_from_edges(rows, rng.integers(0, n, rows.size), n)


# ------------------------------------------------------------------ inputs
def tables(num_cols, D, k, seed, exact):
    """(sp_data f32 [num_cols, k], sp_index u8 [num_cols, k]): distinct ascending selectors;
    values multiples of 0.5 in [-4, 4] (exact) or standard normal."""
    rng = np.random.default_rng(seed)
    sel = np.sort(np.argsort(rng.random((num_cols, D)), axis=1)[:, :k], axis=1).astype(np.uint8)
    if exact:
        data = (rng.integers(-8, 9, (num_cols, k)) * 0.5).astype(np.float32)
    else:
        data = rng.standard_normal((num_cols, k)).astype(np.float32)
    return data, sel


def exact_alpha(H, E, seed):
    return np.random.default_rng(seed).choice(
        np.array([0.25, 0.5, 1.0, 2.0], np.float32), (H, E))


def exact_grad(n, D, seed):
    return (np.random.default_rng(seed).integers(-8, 9, (n, D)) * 0.5).astype(np.float32)


# ------------------------------------------------------------------ float64 restatements
def _edge_terms(ptr, idx, alpha, data, sel, D, left):
    """Per (edge, slot): the features s [E, k], heads [E, k] and the f64 weights alpha[hd(s), e]
    (left=True) or table values (left=False)."""
    H = alpha.shape[0]
    s = sel[idx].astype(np.int64)
    hd = s // (D // H)
    e = np.arange(idx.size)[:, None]
    return s, hd, (alpha[hd, e] if left else data[idx]).astype(np.float64)


def forward64(ptr, idx, alpha, data, sel, D):
    """(out, mag, m) f64 [num_rows, D]: the sums, the sums of |terms| and the nonzero-term
    counts of out[r, s] = sum_e alpha[hd(s), e] * X[idx[e], s]."""
    n = ptr.size - 1
    s, _, w = _edge_terms(ptr, idx, alpha, data, sel, D, True)
    t = w * data[idx].astype(np.float64)
    r = np.broadcast_to(rows_of(ptr)[:, None], s.shape)
    out, mag, m = (np.zeros((n, D)) for _ in range(3))
    np.add.at(out, (r, s), t)
    np.add.at(mag, (r, s), np.abs(t))
    np.add.at(m, (r, s), (t != 0).astype(np.float64))
    return out, mag, m


def backward64(ptr, idx, alpha, grad_out, data, sel, D):
    """((grad_sp, mag, m) f64 [num_cols, k], (grad_alpha, mag, m) f64 [H, E])."""
    H, E = alpha.shape
    num_cols, k = data.shape
    s, hd, w = _edge_terms(ptr, idx, alpha, data, sel, D, True)
    g = grad_out[rows_of(ptr)[:, None], s].astype(np.float64)
    c = np.broadcast_to(idx[:, None], s.shape)
    slot = np.broadcast_to(np.arange(k)[None, :], s.shape)
    ts = w * g
    sp = [np.zeros((num_cols, k)) for _ in range(3)]
    for a, v in zip(sp, (ts, np.abs(ts), (ts != 0).astype(np.float64))):
        np.add.at(a, (c, slot), v)
    ta = data[idx].astype(np.float64) * g
    e = np.broadcast_to(np.arange(E)[:, None], s.shape)
    ga = [np.zeros((H, E)) for _ in range(3)]
    for a, v in zip(ga, (ta, np.abs(ta), (ta != 0).astype(np.float64))):
        np.add.at(a, (hd, e), v)
    return tuple(sp), tuple(ga)


def bound(mag, m):
    """(m + 4) u sum |terms|: any order of m - 1 f32 additions of f32 products, fused or not."""
    return (m + 4.0) * U * mag


def dense_forward64(ptr, idx, alpha, data, sel, D):
    """The same forward as H dense weighted adjacency products on the densified features."""
    n, H = ptr.size - 1, alpha.shape[0]
    num_cols, F = data.shape[0], D // alpha.shape[0]
    X = np.zeros((num_cols, D))
    np.add.at(X, (np.arange(num_cols)[:, None], sel.astype(np.int64)), data.astype(np.float64))
    out = np.zeros((n, D))
    rows = rows_of(ptr)
    for h in range(H):
        A = np.zeros((n, num_cols))
        np.add.at(A, (rows, idx), alpha[h].astype(np.float64))
        out[:, h * F:(h + 1) * F] = A @ X[:, h * F:(h + 1) * F]
    return out


def sequential_f32(terms32):
    """Sum of f32 terms in order with f32 additions (np.add.accumulate keeps the order)."""
    return np.add.accumulate(np.asarray(terms32, np.float32), dtype=np.float32)[-1] \
        if len(terms32) else np.float32(0)
