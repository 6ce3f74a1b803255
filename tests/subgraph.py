"""Shared by tests/test_subgraph_capi.py (CPU) and tests/test_gpu_subgraph.py (GPU): the numpy
restatement of the induced-subgraph extraction of include/maxk_hip.h ("Induced subgraphs"), the
restated kernel names, limits and scratch sizes, the node sets, and float64 torch restatements of
the layers on a subgraph.

The rule is part of the ABI, so the restatement is exact: out_ptr, out_col, out_eid and counts
are compared bit for bit."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import gat_heads as gh
import scan
from gat_heads import ND, NUM, rows_of  # noqa: F401  (used by the test modules)

LIMITS = (16, 512)               # maxk_subgraph_row_limits, asserted against the library
NONE = 2 ** 31 - 1               # local(c) of a node that is not selected
SCAN_TILE = scan.TILE            # positions of a scan tile (csrc/scan.h)
SHARED_KERNELS = ("maxk_sg::mark_init_kernel", "maxk_sg::mark_nodes_kernel")
# the maxk_scan:: kernels of the count: its tile sums also count first positions and strays
SCAN_KERNELS = ("maxk_scan::apply_kernel", "maxk_scan::partials_kernel<3>",
                "maxk_scan::tile_sums_kernel<maxk_sg::PositionItem>")
COUNT_KERNELS = SHARED_KERNELS + SCAN_KERNELS + ("maxk_sg::subgraph_rows_kernel<false>",)
FILL_KERNELS = SHARED_KERNELS + ("maxk_sg::subgraph_rows_kernel<true>",)
KERNELS = tuple(sorted(set(COUNT_KERNELS) | set(FILL_KERNELS)))


def regime(n):
    return 0 if n <= LIMITS[0] else 1 if n <= LIMITS[1] else 2


def scratch_bytes(num_nodes, num_sel):
    """One int32 per node, and three sums per tile of the positions 0 .. num_sel."""
    return 4 * (num_nodes + 3 * ((num_sel + 1 + SCAN_TILE - 1) // SCAN_TILE))


# ------------------------------------------------------------------ the rule
def subgraph_ref(ptr, idx, nodes, num_nodes):
    """(out_ptr int32 [S + 1], out_col int32 [M], out_eid int32 [M], (M, distinct, stray)) of
    maxk_induced_subgraph_count / _fill, transcribed from the header: entries of nodes are
    clamped into [0, num_nodes); local(c) is the lowest position that names c; position i keeps
    the edges of its row whose column is selected, in ascending edge number."""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    raw = np.asarray(nodes, np.int64)
    stray = int(((raw < 0) | (raw >= num_nodes)).sum())
    sel = np.clip(raw, 0, max(num_nodes - 1, 0))
    local = np.full(max(num_nodes, 1), NONE, np.int64)
    for i in range(sel.size - 1, -1, -1):         # the lowest position wins
        local[sel[i]] = i
    distinct = int(sum(local[sel[i]] == i for i in range(sel.size)))
    cols, eids, kept = [], [], []
    for r in sel:
        e = np.arange(ptr[r], ptr[r + 1], dtype=np.int64)
        loc = local[idx[e]]
        keep = loc != NONE
        cols.append(loc[keep])
        eids.append(e[keep])
        kept.append(int(keep.sum()))
    out_ptr = np.zeros(sel.size + 1, np.int64)
    np.cumsum(kept, out=out_ptr[1:])
    col = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    eid = np.concatenate(eids) if eids else np.zeros(0, np.int64)
    return (out_ptr.astype(np.int32), col.astype(np.int32), eid.astype(np.int32),
            (int(out_ptr[-1]), distinct, stray))


def count_ref(ptr, idx, nodes, num_nodes):
    """(out_ptr int32 [S + 1], (M, distinct, stray)) of maxk_induced_subgraph_count without a
    loop over the positions, for selections too long for subgraph_ref."""
    raw = np.asarray(nodes, np.int64)
    stray = int(((raw < 0) | (raw >= num_nodes)).sum())
    sel = np.clip(raw, 0, max(num_nodes - 1, 0))
    named = np.unique(sel)
    selected = np.zeros(max(num_nodes, 1), bool)
    selected[named] = True
    kept_of_row = np.bincount(rows_of(ptr), weights=selected[np.asarray(idx, np.int64)],
                              minlength=num_nodes).astype(np.int64)
    out_ptr = np.zeros(sel.size + 1, np.int64)
    np.cumsum(kept_of_row[sel], out=out_ptr[1:])
    return out_ptr.astype(np.int32), (int(out_ptr[-1]), int(named.size), stray)


def dense_of(ptr, idx, num_cols, val=None):
    """float64 [rows, num_cols]: the matrix of a CSR structure (repeated pairs add)."""
    a = np.zeros((ptr.size - 1, num_cols))
    v = np.ones(idx.size) if val is None else np.asarray(val, np.float64)
    np.add.at(a, (rows_of(ptr), idx), v)
    return a


# ------------------------------------------------------------------ graph and node sets
def graph():
    """(ptr, idx, N): the 600 x 600 graph of the multi-head tests. Rows 0 .. ND - 1 are the
    designed ones (lengths 0, 0, 1, 2, 15, 16, 17, 511, 512, 513, 100 and the hub row of 5,000)
    and take their columns from the undesigned nodes ND .. N - 1."""
    return gh.graph_arrays() + (NUM,)


DESIGNED_ROWS = tuple(range(ND))
HUB = ND - 1


@functools.lru_cache(maxsize=None)
def node_sets():
    """name -> int32 nodes. `designed` selects the designed rows and none of their columns
    (nothing kept), `few_columns` adds 40 undesigned nodes, `every_column` every column of the
    designed rows (every edge of theirs kept)."""
    ptr, idx, n = graph()
    rng = np.random.default_rng(18)
    designed = np.array(DESIGNED_ROWS, np.int64)
    cols = np.unique(np.concatenate([idx[ptr[r]:ptr[r + 1]] for r in DESIGNED_ROWS]))
    few = rng.choice(np.arange(ND, n), 40, replace=False)
    sets = {"none": np.zeros(0, np.int64),
            "isolated": np.array([0]),
            "hub": np.array([HUB]),
            "all": np.arange(n),
            "permuted": rng.permutation(n),
            "half": np.sort(rng.choice(n, n // 2, replace=False)),
            "designed": designed,
            "few_columns": rng.permutation(np.concatenate([designed, few])),
            "every_column": np.concatenate([cols, designed])}
    out = {k: v.astype(np.int32) for k, v in sets.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """subgraph_ref of the node set `name`, computed once."""
    ptr, idx, n = graph()
    return subgraph_ref(ptr, idx, node_sets()[name], n)


def kept_fractions():
    """{(regime, kind)} over every selected row of every node set: kind is "nothing", "some" or
    "all" of a row with at least one edge; and the set of selected row lengths."""
    ptr, _, _ = graph()
    seen, lengths = set(), set()
    for name, nodes in node_sets().items():
        out_ptr = reference(name)[0]
        for i, r in enumerate(nodes):
            n, kept = int(ptr[r + 1] - ptr[r]), int(out_ptr[i + 1] - out_ptr[i])
            lengths.add(n)
            if n:
                seen.add((regime(n), "nothing" if kept == 0 else "all" if kept == n else "some"))
    return seen, lengths


# ------------------------------------------------------------------ layers, float64
def masked64(x, sel):
    return torch.zeros_like(x).scatter(1, sel, x.gather(1, sel))


def aggregate64(ptr, idx, values, x):
    """sum over each row's edges of values[e] * x[idx[e]], float64 torch."""
    rows = torch.from_numpy(rows_of(ptr))
    msg = x[torch.from_numpy(idx.astype(np.int64))] * values[:, None]
    return torch.zeros(ptr.size - 1, x.shape[1], dtype=torch.float64).index_add(0, rows, msg)


def degree_values(ptr, idx, kind):
    """The edge values CSRGraph.edge_values(kind) stands for, float64, from the structure's own
    degrees (clamped to >= 1)."""
    n = ptr.size - 1
    ind = np.maximum(np.diff(ptr), 1).astype(np.float64)
    outd = np.maximum(np.bincount(idx, minlength=n), 1).astype(np.float64)
    rows = rows_of(ptr)
    v = {"sum": np.ones(idx.size), "mean": 1 / ind[rows],
         "both": outd[idx] ** -0.5 * ind[rows] ** -0.5}[kind]
    return torch.from_numpy(v)


def given_max64(ptr, idx, X, arg_edge):
    """max over each row's edges of X[idx[e]] with the winners given (arg_edge [N, D], -1: the
    implicit zero): a gather, so the gradient goes to the winner alone. The given winners are
    checked: no message of the row beats them by more than rounding."""
    ae = arg_edge.cpu().long()
    col = torch.from_numpy(idx.astype(np.int64))[ae.clamp(min=0)]
    out = torch.where(ae >= 0, X.gather(0, col), torch.zeros_like(X))
    rows = torch.from_numpy(rows_of(ptr))
    msg = X.detach()[torch.from_numpy(idx.astype(np.int64))]
    best = torch.full(X.shape, -float("inf"), dtype=torch.float64)
    best = best.scatter_reduce(0, rows[:, None].expand_as(msg), msg, "amax", include_self=True)
    best = torch.where(torch.isinf(best), torch.zeros_like(best), best)
    assert float((best - out.detach()).abs().max()) <= 1e-5 * float(best.abs().max())
    return out


def layer64(kind, layer, ptr, idx, feat, given, edge_weight=None):
    """(out, parameters, edge_weight) of the layer `kind` in float64 torch on the CPU, on the
    structure (ptr, idx) with its own degrees. `given` holds what is discrete in the f32 run:
    the top-k selections ("sel", and "sel_pool" after fc_pool) and the winners of the pool
    maximum ("arg_edge"). The parameters (and edge_weight) require gradients."""
    p = {n: v.detach().double().cpu().requires_grad_(True) for n, v in layer.named_parameters()}
    x = feat.detach().double().cpu()
    w = None if edge_weight is None else edge_weight.detach().double().cpu().requires_grad_(True)
    sel = given["sel"].cpu().long()
    if kind in ("sage_mean", "sage_gcn", "sage_pool"):
        xm = masked64(x, sel)
        if kind == "sage_mean":
            neigh = aggregate64(ptr, idx, degree_values(ptr, idx, "mean"), xm)
            out = xm @ p["fc_self.weight"].t() + neigh @ p["fc_neigh.weight"].t() + p["bias"]
        elif kind == "sage_gcn":
            neigh = aggregate64(ptr, idx, degree_values(ptr, idx, "sum"), xm)
            deg = torch.from_numpy(np.diff(ptr).astype(np.float64) + 1)[:, None]
            out = ((neigh + xm) / deg) @ p["fc_neigh.weight"].t() + p["bias"]
        else:
            h = masked64(xm @ p["fc_pool.weight"].t() + p["fc_pool.bias"],
                         given["sel_pool"].cpu().long())
            neigh = given_max64(ptr, idx, h, given["arg_edge"])
            out = xm @ p["fc_self.weight"].t() + neigh @ p["fc_neigh.weight"].t() + p["bias"]
    elif kind == "gcn":
        values = degree_values(ptr, idx, "both")
        if w is not None:
            values = values * w
        out = aggregate64(ptr, idx, values, masked64(x @ p["weight"], sel)) + p["bias"]
    elif kind == "gin":
        xm = masked64(x, sel)
        out = (1 + p["eps"]) * xm + aggregate64(ptr, idx, degree_values(ptr, idx, "sum"), xm)
    elif kind == "gat":
        H, Fo = layer.num_heads, layer.out_feats
        rows = torch.from_numpy(rows_of(ptr))
        cols = torch.from_numpy(idx.astype(np.int64))
        n = ptr.size - 1
        h = x @ p["fc.weight"].t()
        hv = h.view(-1, H, Fo)
        el = (hv * p["attn_l"]).sum(-1).t()
        er = (hv * p["attn_r"]).sum(-1).t()
        e = F.leaky_relu(el[:, cols] + er[:, rows], layer.negative_slope)
        m = torch.full((H, n), -float("inf"), dtype=torch.float64)
        m = m.scatter_reduce(1, rows.expand(H, -1), e.detach(), "amax")
        ex = torch.exp(e - m[:, rows])
        alpha = ex / torch.zeros(H, n, dtype=torch.float64).index_add(1, rows, ex)[:, rows]
        xm = masked64(h, sel)
        wide = alpha.t().repeat_interleave(Fo, dim=1)       # [E, D]: the head's alpha per feature
        out = torch.zeros_like(h).index_add(0, rows, wide * xm[cols]) + p["bias"]
        if H > 1:
            out = out.view(-1, H, Fo)
    else:
        raise ValueError(kind)
    return out, p, w
