"""Shared by tests/test_max_aggregate_capi.py (CPU) and tests/test_gpu_max_aggregate.py (GPU): the
restatements of include/maxk_hip.h ("Max aggregation") in numpy on the host, the inputs, and the
restated selectors of csrc/variants_max.h. The graph, the transposed structure and the table
generators are those of tests/gat_heads.py.

The forward is restated on value keys, not floats: key(x) is the order of the exact top-k (any
NaN above +Inf, +0.0 above -0.0, else numeric), so the restatement ranks exactly what the
contract ranks and returns the winner's own bits."""
import functools

import numpy as np

import gat_heads as gh
from gat_heads import (NUM, bound, exact_grad, graph_arrays, rows_of, small_graph,  # noqa: F401
                       tables, transposed)

LIMITS = (16, 512, 16, 512)      # maxk_max_row_limits, asserted against the library by the tests
assert LIMITS == gh.LIMITS       # the 600 x 600 graph is designed around these
KEY_ZERO = np.uint32(0x80000000)  # key(+0.0f)

# (D, k) with MaxK tables, and with identity selectors (k = D)
TABLE_SHAPES = ((256, 16), (256, 32), (64, 8), (100, 10), (256, 64), (256, 100), (256, 1))
IDENTITY_SHAPES = ((256, 256), (8, 8))
SHAPES = TABLE_SHAPES + IDENTITY_SHAPES


# ------------------------------------------------------------------ selectors, restated
def max_lanes(k):
    lp = 8
    while lp < k and lp < 64:
        lp *= 2
    return lp


def fwd_kernel_name(k, arg):
    return f"maxk_mx::max_fwd_kernel<{max_lanes(k)}, {'true' if arg else 'false'}>"


def bwd_kernel_name(k):
    return f"maxk_mx::max_bwd_kernel<{max_lanes(k)}>"


# ------------------------------------------------------------------ value keys
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def order_key(x):
    """u32 keys of f32 values: larger value, larger key; +0.0 above -0.0; every NaN the largest."""
    b = bits(x)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000), np.uint32(0xffffffff),
                    key).astype(np.uint32)


# ------------------------------------------------------------------ restatements
def _candidates(ptr, idx, data, sel, D):
    """Every explicit candidate, flat over (edge, slot): its row, feature, place j of the edge in
    its row, slot, edge, key, and the group r * D + s."""
    E, k = idx.size, data.shape[1]
    r = np.repeat(rows_of(ptr), k)
    e = np.repeat(np.arange(E, dtype=np.int64), k)
    j = e - ptr[r].astype(np.int64)
    l = np.tile(np.arange(k, dtype=np.int64), E)
    c = idx[e].astype(np.int64)
    s = sel[c, l].astype(np.int64)
    key = order_key(data[c, l])
    return dict(r=r, s=s, j=j, l=l, e=e, c=c, key=key, grp=r * D + s)


def _winners(cand):
    """Positions (into the flat candidates) of each group's winner, the groups' ids, and the
    candidates sorted so that a group's come together, best first: highest key, then lowest j,
    then lowest l."""
    primary = (cand["grp"].astype(np.uint64) << np.uint64(32)) | \
        (np.uint64(0xffffffff) - cand["key"].astype(np.uint64))
    order = np.lexsort((cand["j"] * 256 + cand["l"], primary))
    g = cand["grp"][order]
    first = np.ones(g.size, bool)
    first[1:] = g[1:] != g[:-1]
    return order[first], g[first], order, first


def _analyse(ptr, idx, data, sel, D):
    """The candidates, their ranking and, per (r, s) group, the number of distinct edges that
    select s: what forward_ref and classes both start from."""
    cand = _candidates(ptr, idx, data, sel, D)
    win, grp, order, first = _winners(cand)
    pairs = np.unique(cand["grp"] * np.int64(idx.size) + cand["e"])
    hit_grp, hits = np.unique(pairs // idx.size, return_counts=True)
    assert np.array_equal(hit_grp, grp)
    return cand, win, grp, order, first, hits


def forward_ref(ptr, idx, data, sel, D, pre=None):
    """(out f32, arg_edge int32, arg_slot u8), each [num_rows, D]: the semantics of the
    header, restated. Explicit candidates are ranked by (key, -j, -l); the implicit +0.0f
    competes where fewer distinct edges select the feature than the row has, and loses a tie.
    `pre`: _analyse of the same arguments, when the caller has it."""
    n = ptr.size - 1
    out = np.zeros(n * D, np.uint32)
    ae = np.full(n * D, -1, np.int32)
    sl = np.zeros(n * D, np.uint8)
    if idx.size:
        cand, win, grp, _, _, hits = pre or _analyse(ptr, idx, data, sel, D)
        rowlen = np.diff(ptr).astype(np.int64)[grp // D]
        explicit = ~((hits < rowlen) & (cand["key"][win] < KEY_ZERO))
        w, gsel = win[explicit], grp[explicit]
        out[gsel] = bits(data[cand["c"][w], cand["l"][w]])
        ae[gsel] = cand["e"][w]
        sl[gsel] = cand["l"][w]
    return out.view(np.float32).reshape(n, D), ae.reshape(n, D), sl.reshape(n, D)


def dense_ref(ptr, idx, data, sel, D):
    """The same by densifying (without adding repeats: tables with distinct selectors only) and
    taking each row's maximum over its edges: a dense [num_cols, D] rank matrix in which an
    explicit value ranks 2 * key + 1 and the implicit zero 2 * key(+0.0), the first edge that
    attains the row's best wins."""
    n, (num_cols, k) = ptr.size - 1, data.shape
    assert all(np.unique(row).size == k for row in sel)
    rank = np.full((num_cols, D), 2 * np.int64(KEY_ZERO), np.int64)
    slot = np.full((num_cols, D), -1, np.int64)
    cols = np.arange(num_cols)[:, None]
    rank[cols, sel] = 2 * order_key(data).astype(np.int64) + 1
    slot[cols, sel] = np.arange(k)[None, :]
    out = np.zeros((n, D), np.uint32)
    ae = np.full((n, D), -1, np.int32)
    sl = np.zeros((n, D), np.uint8)
    feat = np.arange(D)
    for r in range(n):
        seg = idx[ptr[r]:ptr[r + 1]]
        if seg.size == 0:
            continue
        j = np.argmax(rank[seg], axis=0)            # the first edge of the best rank
        c = seg[j]
        ex = slot[c, feat] >= 0
        l = np.where(ex, slot[c, feat], 0)
        out[r] = np.where(ex, bits(data[c, l]), 0)
        ae[r] = np.where(ex, ptr[r] + j, -1)
        sl[r] = l
    return out.view(np.float32), ae, sl


def backward64(ptr, idx, grad_out, arg_edge, arg_slot, sel):
    """(grad_sp, mag, m) f64 [num_cols, k]: the sums, the sums of |terms| and the nonzero-term
    counts of grad_sp[c, l] = sum_j [arg_edge[r, s] == e and arg_slot[r, s] == l] grad_out[r, s],
    over every edge e of column c with r its row and s = sel[c, l]."""
    num_cols, k = sel.shape
    E = idx.size
    r = rows_of(ptr)[:, None]
    e = np.arange(E)[:, None]
    l = np.arange(k)[None, :]
    c = idx.astype(np.int64)[:, None]
    s = sel[idx].astype(np.int64)
    match = (arg_edge[r, s] == e) & (arg_slot[r, s] == l)
    t = np.where(match, grad_out[r, s].astype(np.float64), 0.0)
    res = [np.zeros((num_cols, k)) for _ in range(3)]
    cc, ll = np.broadcast_to(c, s.shape), np.broadcast_to(l, s.shape)
    for a, v in zip(res, (t, np.abs(t), (t != 0).astype(np.float64))):
        np.add.at(a, (cc, ll), v)
    return tuple(res)


# ------------------------------------------------------------------ inputs
def identity_tables(num_cols, D, seed, exact):
    rng = np.random.default_rng(seed)
    if exact:
        data = (rng.integers(-8, 9, (num_cols, D)) * 0.5).astype(np.float32)
    else:
        data = rng.standard_normal((num_cols, D)).astype(np.float32)
    return data, np.tile(np.arange(D, dtype=np.uint8), (num_cols, 1))


def case_tables(D, k, exact, seed=0):
    """The tables of shape (D, k): MaxK-like tables (distinct ascending selectors), identity
    selectors where k = D on the identity shapes."""
    if (D, k) in IDENTITY_SHAPES:
        return identity_tables(NUM, D, seed + D + k, exact)
    return tables(NUM, D, k, seed + D + k, exact)


def repeated_tables(D, k, seed):
    """Exact tables in which, in every third column, three slots repeat the selector of another
    slot, one of them with that slot's value as well (equal candidates of one edge)."""
    data, sel = tables(NUM, D, k, seed, exact=True)
    rng = np.random.default_rng(seed + 1)
    data, sel = data.copy(), sel.copy()
    for c in range(0, NUM, 3):
        dst = rng.choice(k, 3, replace=False)
        src = rng.integers(0, k, 3)
        sel[c, dst] = sel[c, src]
        if dst[0] != src[0]:
            data[c, dst[0]] = data[c, src[0]]
    return data, sel


def padded_tables(D, k, seed):
    """ref_compat-style tables: every other column fills only its first slots, the rest are
    (0.0f, 0) padding slots, which here are explicit candidates for feature 0."""
    data, sel = tables(NUM, D, k, seed, exact=True)
    data, sel = data.copy(), sel.copy()
    fill = np.random.default_rng(seed + 2).integers(1, k + 1, NUM)
    fill[1::2] = k
    pad = np.arange(k)[None, :] >= fill[:, None]
    data[pad], sel[pad] = 0.0, 0
    return data, sel


def exact_analysis(D, k):
    """(data, sel, _analyse of them) of shape (D, k)'s tie-heavy exact tables on the 600-row graph."""
    ptr, idx = graph_arrays()
    data, sel = case_tables(D, k, exact=True)
    return data, sel, _analyse(ptr, idx, data, sel, D)


@functools.lru_cache(maxsize=None)
def exact_case(D, k):
    """(data, sel, out, arg_edge, arg_slot) of the tie-heavy exact tables on the 600-row graph."""
    ptr, idx = graph_arrays()
    data, sel, pre = exact_analysis(D, k)
    res = (data, sel) + forward_ref(ptr, idx, data, sel, D, pre)
    for a in res:
        a.setflags(write=False)
    return res


def classes(ptr, idx, data, sel, D, out, arg_edge, arg_slot, pre=None):
    """Which kinds of output element occur, as a dict of booleans (the precondition of the GPU
    tests): `implicit` an implicit zero wins in a row with edges; `negative` an explicit negative
    value wins (every neighbour selected the feature); `zero_tie` an explicit 0.0 wins where the
    implicit zero competes; `edge_tie` equal best candidates in edges of different columns;
    `multi_edge_tie` equal best candidates in two edges of the winner's column; `slot_tie` equal
    best candidates in two slots of one edge."""
    cand, win, grp, order, first, hits = pre or _analyse(ptr, idx, data, sel, D)
    rowlen = np.diff(ptr)
    nonempty = np.repeat(rowlen > 0, D).reshape(-1, D)
    full = hits == rowlen[grp // D]
    o, ae = out.reshape(-1), arg_edge.reshape(-1)
    wkey = cand["key"][win]
    # candidates of each group that tie with its winner
    gidx = np.cumsum(first) - 1                       # group number of each sorted candidate
    top = (cand["key"][order] == wkey[gidx]) & (ae[grp] >= 0)[gidx]
    wj, wc = cand["j"][win][gidx], cand["c"][win][gidx]
    sj, sc = cand["j"][order], cand["c"][order]
    return dict(
        implicit=bool(((arg_edge == -1) & nonempty).any()),
        negative=bool(((o[grp] < 0) & (ae[grp] >= 0) & full).any()),
        zero_tie=bool(((wkey == KEY_ZERO) & ~full & (ae[grp] >= 0)).any()),
        edge_tie=bool((top & (sj != wj) & (sc != wc)).any()),
        multi_edge_tie=bool((top & (sj != wj) & (sc == wc)).any()),
        slot_tie=bool((top & (sj == wj) & ~first).any()),
    )


# ------------------------------------------------------------------ moved rows
def moved_graph(segs, starts, seed, num_cols=NUM):
    """A graph of another size in which the given segments (arrays of column indices) are rows
    at other positions, each starting at an edge offset with ptr % 4 == its wanted start:
    (ptr, idx, the rows' positions)."""
    rng = np.random.default_rng(seed)
    rows, cols, where = [], [], []
    r = total = 0
    for seg, start in zip(segs, starts):
        while total % 4 != start:       # filler rows of one edge shift the segment's start
            rows.append(np.array([r]))
            cols.append(rng.integers(0, num_cols, 1))
            r += 1
            total += 1
        rows.append(np.full(len(seg), r))
        cols.append(np.asarray(seg))
        where.append(r)
        total += len(seg)
        r += 1
    ptr, idx = gh.csr_from_edges(np.concatenate(rows), np.concatenate(cols), r + 7)
    return ptr, idx, where
