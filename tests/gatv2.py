"""Shared by tests/test_gatv2_capi.py (CPU) and tests/test_gpu_gatv2.py (GPU): float64 restatements
of the formulas of include/maxk_hip.h ("MaxK GATv2 attention") with their bounds, and the model in
float64 torch. Graphs, tables and helpers are those of tests/gat_heads.py. The slope enters as the
f32 value the kernels get, so the restatements see the same inputs."""
import numpy as np
import torch
import torch.nn.functional as F

import gat_heads as gh

U = gh.U
SLOPE = float(np.float32(0.2))
# every lanes(k), both head-place counts, k = D
SHAPES = ((64, 1, 8), (64, 4, 16), (96, 3, 96), (256, 8, 32), (256, 16, 16), (256, 4, 255))
MAX_PARTIALS, TILE = 1024, 16


def lrelu(t, slope=SLOPE):
    return np.where(t > 0, t, slope * t)


def dlrelu(t, slope=SLOPE):
    return np.where(t > 0, 1.0, slope)


def inputs(num_rows, num_cols, num_edges, D, H, k, seed):
    """(sp_data, sp_index, fd [num_rows, D], attn [H, F], g [H, E]) f32, standard normal."""
    data, sel = gh.tables(num_cols, D, k, seed, exact=False)
    rng = np.random.default_rng(seed + 1)
    fd, attn, g = (rng.standard_normal(s).astype(np.float32)
                   for s in ((num_rows, D), (H, D // H), (H, num_edges)))
    return data, sel, fd, attn, g


def _slots(ptr, idx, data, sel, fd, attn):
    """Per (edge, slot), [E, k]: row, feature, head, and f64 x, fd[v, s], attn[s]."""
    rows = np.broadcast_to(gh.rows_of(ptr)[:, None], (idx.size, sel.shape[1]))
    s = sel[idx].astype(np.int64)
    hd = s // attn.shape[1]
    return rows, s, hd, data[idx].astype(np.float64), fd[rows, s].astype(np.float64), \
        attn.reshape(-1)[s].astype(np.float64)


def _sums(shape, where, term, mag):
    """(sum, sum |terms|, nonzero-term count) of the terms scattered to `where`."""
    out = [np.zeros(shape) for _ in range(3)]
    for a, v in zip(out, (term, mag, (term != 0).astype(np.float64))):
        np.add.at(a, where, v)
    return tuple(out)


def score64(ptr, idx, data, sel, fd, attn):
    """(Delta, mag, m) f64 [H, E]; a term's magnitude is |attn| (|lrelu(x + fd)| + |lrelu(fd)|)."""
    _, _, hd, x, f, a = _slots(ptr, idx, data, sel, fd, attn)
    e = np.broadcast_to(np.arange(idx.size)[:, None], hd.shape)
    return _sums((attn.shape[0], idx.size), (hd, e), a * (lrelu(x + f) - lrelu(f)),
                 np.abs(a) * (np.abs(lrelu(x + f)) + np.abs(lrelu(f))))


def backward64(ptr, idx, data, sel, fd, attn, g):
    """((grad_sp, mag, m) [num_cols, k], (grad_fd, mag, m) [num_rows, D], (grad_attn, mag, m)
    [D]) f64. grad_attn's terms have the forward's magnitudes (the same difference of two rounded
    values), and its m is the most terms of one work-group's partial plus the partials."""
    rows, s, hd, x, f, a = _slots(ptr, idx, data, sel, fd, attn)
    n, D = fd.shape
    gv = g[hd, np.arange(idx.size)[:, None]].astype(np.float64)
    slot = np.broadcast_to(np.arange(sel.shape[1])[None, :], s.shape)
    c = np.broadcast_to(idx[:, None], s.shape)
    t = a * gv * dlrelu(x + f)
    sp = _sums(data.shape, (c, slot), t, np.abs(t))
    t = gv * a * (dlrelu(x + f) - dlrelu(f))
    gfd = _sums((n, D), (rows, s), t, np.abs(t))
    ga, gmag, _ = _sums((D,), (s,), gv * (lrelu(x + f) - lrelu(f)),
                        np.abs(gv) * (np.abs(lrelu(x + f)) + np.abs(lrelu(f))))
    parts = min((n + TILE - 1) // TILE, MAX_PARTIALS)
    per = np.zeros((parts, D))
    np.add.at(per, ((rows // TILE) % parts, s), 1.0)
    return sp, gfd, (ga, gmag, per.max(0) + parts)


def bound(mag, m):
    """(m + 6) u sum |terms| (include/maxk_hip.h)."""
    return (m + 6.0) * U * mag


def worst(got, want, mag, m):
    """The largest error / bound; an element with no terms must be exactly zero."""
    err, bnd = np.abs(got.astype(np.float64) - want), bound(mag, m)
    assert not (err[bnd == 0] != 0).any()
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0


def model64(ptr, idx, feat, p, H, sp_index=None, slope=SLOPE):
    """The layer in float64 torch, out [N, H, F]. p: w_src, b_src, w_dst, b_dst [D, in] / [D] and
    attn [H, F]. sp_index None: dglnn.GATv2Conv's formula on the dense fs; else the MaxK model
    with the rows' kept features given."""
    rows = torch.from_numpy(gh.rows_of(ptr).astype(np.int64))
    cols = torch.from_numpy(idx.astype(np.int64))
    fs = feat @ p["w_src"].T + p["b_src"]
    fd = feat @ p["w_dst"].T + p["b_dst"]
    (N, D), a = fs.shape, p["attn"].reshape(-1)
    if sp_index is None:
        xs = fs
        e = a * F.leaky_relu(fs[cols] + fd[rows], slope)
    else:
        mask = torch.zeros(N, D, dtype=fs.dtype).scatter_(1, sp_index.long(), 1.0)
        xs = fs * mask
        z = fd[rows]
        e = a * (F.leaky_relu(xs[cols] + z, slope) - F.leaky_relu(z, slope)) * mask[cols]
    e = e.view(-1, H, D // H).sum(-1)
    top = torch.full((N, H), -np.inf, dtype=fs.dtype).scatter_reduce(
        0, rows[:, None].expand(-1, H), e.detach(), "amax")
    w = torch.exp(e - top[rows])
    alpha = w / torch.zeros(N, H, dtype=fs.dtype).index_add_(0, rows, w)[rows]
    return torch.zeros(N, H, D // H, dtype=fs.dtype).index_add_(
        0, rows, alpha[:, :, None] * xs[cols].view(-1, H, D // H))
