"""GATv2 on MaxK features: attention scored on the kept features, in HIP.

    fs = fc_src(feat);  fd = fc_dst(feat)                 (or fc_src, with share_weights)
    (sp_data, sp_index) = MaxK_k(fs)
    Delta[h, e] = sum_{l: s // F == h} attn[s] * (lrelu(sp_data[u, l] + fd[v, s]) - lrelu(fd[v, s]))
    alpha = edge_softmax_heads(Delta)                     e = u -> v, s = sp_index[u, l]
    out[v] = sum_{u -> v} alpha[s // F, e] * xs[u, s]     (heads_aggregate)

GATv2's score ``sum_f attn[h, f] * lrelu(xs[u, h, f] + fd[v, h, f])`` differs from ``Delta`` by a
term that depends on ``v`` alone, which the softmax over ``v``'s in-edges removes: ``k`` gathered
terms per edge instead of an ``[E, H, F]`` tensor. At ``k = D`` the layer is ``dglnn.GATv2Conv``
without residual or activation.

* :func:`edge_softmax_heads`: the edge softmax of head-major ``[H, E]`` logits, every head in one
  launch, forward and backward.
* :func:`gatv2_attention`: ``alpha [H, E]`` from the MaxK tables, ``fd`` and ``attn``; the
  backward is the softmax backward, one kernel over the rows (``grad_fd``, ``grad_attn``) and one
  over the columns (``grad_sp_data``), each skipped when nothing needs it.
* :class:`MaxKGATv2Conv`: the layer.

All backwards are first order only (:func:`maxk_kernels.autograd.first_order_only`).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .autograd import CSRGraph, first_order_only, maxk
from .heads import heads_aggregate
from .sampling import Block


class EdgeSoftmaxHeadsFunction(torch.autograd.Function):
    """``ops.edge_softmax_heads`` forward, ``ops.edge_softmax_backward_heads`` backward; only the
    output is saved."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, logits: torch.Tensor):
        y = ops.edge_softmax_heads(graph.ptr, logits.contiguous())
        ctx.save_for_backward(y)
        ctx.graph = graph
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @first_order_only
    def backward(ctx, grad_y):
        if grad_y is None or not ctx.needs_input_grad[1]:
            return None, None
        (y,) = ctx.saved_tensors
        return None, ops.edge_softmax_backward_heads(ctx.graph.ptr, y, grad_y.contiguous())


def _check_heads(graph: CSRGraph, t, name: str) -> None:
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and
            t.shape[0] >= 1 and t.shape[1] == graph.num_edges and t.device == graph.device):
        raise RuntimeError(f"{name} must be a float32 [num_heads, num_edges] tensor on the "
                           "graph's device, in the CSRGraph's edge order")


def edge_softmax_heads(graph: CSRGraph, logits: torch.Tensor) -> torch.Tensor:
    """:func:`maxk_kernels.edge_softmax` of every row of head-major ``logits [H, E]``,
    differentiable in ``logits``; row ``h`` is the single-head call bit for bit."""
    _check_heads(graph, logits, "logits")
    return EdgeSoftmaxHeadsFunction.apply(graph, logits)


class GATv2AttentionFunction(torch.autograd.Function):
    """``alpha [H, E]`` from ``sp_data``, ``sp_index``, ``fd``, ``attn`` on a CSRGraph. Saved:
    ``alpha`` and the inputs (the logits are not kept). The row kernel runs only when ``fd`` or
    ``attn`` needs a gradient, the column kernel only when ``sp_data`` does."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, sp_data, sp_index, fd, attn, negative_slope: float):
        fd, attn = ops._rows_in_place(fd), attn.contiguous()
        logits = ops.gatv2_score(graph.ptr, graph.idx, sp_data, sp_index, fd, attn, negative_slope)
        alpha = ops.edge_softmax_heads(graph.ptr, logits)
        ctx.save_for_backward(alpha, sp_data, sp_index, fd, attn)
        ctx.graph = graph
        ctx.negative_slope = float(negative_slope)
        ctx.set_materialize_grads(False)
        return alpha

    @staticmethod
    @first_order_only
    def backward(ctx, grad_alpha):
        need_sp, need_fd, need_attn = (ctx.needs_input_grad[i] for i in (1, 3, 4))
        if grad_alpha is None or not (need_sp or need_fd or need_attn):
            return (None,) * 6
        alpha, sp_data, sp_index, fd, attn = ctx.saved_tensors  # read once
        graph, slope = ctx.graph, ctx.negative_slope
        g = ops.edge_softmax_backward_heads(graph.ptr, alpha, grad_alpha.contiguous())
        grad_sp = grad_fd = grad_attn = None
        if need_fd or need_attn:
            grad_fd, grad_attn = ops.gatv2_score_backward_rows(
                graph.ptr, graph.idx, sp_data, sp_index, fd, attn, slope, g)
        if need_sp:
            ptr_t, idx_t, _ = graph.transposed_structure()
            grad_sp = ops.gatv2_score_backward_cols(ptr_t, idx_t, graph.transposed_order(),
                                                    sp_data, sp_index, fd, attn, slope, g)
        return (None, grad_sp, None, grad_fd if need_fd else None,
                grad_attn if need_attn else None, None)


def gatv2_attention(graph: CSRGraph, sp_data: torch.Tensor, sp_index: torch.Tensor,
                    fd: torch.Tensor, attn: torch.Tensor,
                    negative_slope: float = 0.2) -> torch.Tensor:
    """Attention weights ``alpha [H, E]`` of GATv2 on MaxK features, in the CSRGraph's own edge
    order: ``sp_data`` f32 / ``sp_index`` u8 ``[N, k]`` the MaxK tables of the source side, ``fd``
    f32 ``[N, D]`` the destination side, ``attn`` f32 ``[H, D // H]``. Differentiable in
    ``sp_data``, ``fd`` and ``attn``; ``alpha`` is what :func:`maxk_kernels.heads_aggregate`
    takes."""
    if not (isinstance(attn, torch.Tensor) and attn.dim() == 2 and isinstance(fd, torch.Tensor) and
            fd.dim() == 2 and attn.numel() == fd.shape[1]):
        raise RuntimeError("attn must be [num_heads, D // num_heads] for fd [num_nodes, D]")
    if fd.shape[0] != graph.num_nodes:
        raise RuntimeError("fd must have one row per node of the graph")
    return GATv2AttentionFunction.apply(graph, sp_data, sp_index, fd, attn, float(negative_slope))


class MaxKGATv2Conv(nn.Module):
    """``dglnn.GATv2Conv`` without residual or activation on MaxK features, ``[N, in_feats] ->
    [N, num_heads, out_feats]`` (the model of the module's docstring). MaxK keeps ``maxk``
    features of the whole ``num_heads * out_feats <= 256`` row of ``fc_src(feat)``; with
    ``maxk = num_heads * out_feats`` the layer computes what DGL's does. ``feat_drop`` is
    ``F.dropout`` on the input and ``attn_drop`` on ``alpha``, as in DGL; ``share_weights`` uses
    ``fc_src`` for both sides. The attention needs the CSRGraph's own edge order."""

    def __init__(self, in_feats, out_feats, num_heads, maxk=32, feat_drop=0., attn_drop=0.,
                 negative_slope=0.2, bias=True, share_weights=False, allow_zero_in_degree=False,
                 topk_mode="exact"):
        super().__init__()
        self.num_heads = int(num_heads)
        if self.num_heads < 1:
            raise ValueError(f"num_heads must be >= 1, got {num_heads}")
        d = self.num_heads * out_feats
        if d > 256 or d % 4 != 0:
            raise ValueError("num_heads * out_feats = D must be a multiple of 4, at most 256 "
                             f"(u8 selectors), got {d}")
        self.in_feats, self.out_feats = in_feats, out_feats
        self.maxk = maxk
        self.feat_drop, self.attn_drop = float(feat_drop), float(attn_drop)
        self.negative_slope = float(negative_slope)
        self.share_weights = bool(share_weights)
        self.allow_zero_in_degree = allow_zero_in_degree
        self.topk_mode = topk_mode
        self.fc_src = nn.Linear(in_feats, d, bias=bias)
        self.fc_dst = self.fc_src if share_weights else nn.Linear(in_feats, d, bias=bias)
        self.attn = nn.Parameter(torch.empty(self.num_heads, out_feats))
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        for fc in (self.fc_src,) if self.share_weights else (self.fc_src, self.fc_dst):
            nn.init.xavier_normal_(fc.weight, gain=gain)
            if fc.bias is not None:
                nn.init.zeros_(fc.bias)
        nn.init.xavier_normal_(self.attn, gain=gain)

    def forward(self, graph, feat: torch.Tensor) -> torch.Tensor:
        if isinstance(graph, Block) or (isinstance(graph, (list, tuple)) and graph and
                                        all(isinstance(b, Block) for b in graph)):
            raise NotImplementedError("MaxKGATv2Conv does not take a Block")
        if not isinstance(graph, CSRGraph):
            raise TypeError("MaxKGATv2Conv needs a maxk_kernels.CSRGraph: the attention weights "
                            "follow the CSRGraph's own edge order")
        if not self.allow_zero_in_degree and bool((graph.in_degrees() == 0).any()):
            raise ValueError("Graph has nodes with zero in-degree")
        h = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
        fs = self.fc_src(h)
        fd = fs if self.share_weights else self.fc_dst(h)
        sp_data, sp_index = maxk(fs, self.maxk, self.topk_mode)
        alpha = gatv2_attention(graph, sp_data, sp_index, fd, self.attn, self.negative_slope)
        if self.attn_drop > 0:
            alpha = F.dropout(alpha, self.attn_drop, self.training)
        rst = heads_aggregate(graph, alpha, sp_data, sp_index, fs.shape[1])
        return rst.view(-1, self.num_heads, self.out_feats)
