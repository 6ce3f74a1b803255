"""Multi-head GAT on MaxK features: head-batched attention and the fused multi-head aggregation.

    alpha[h] = edge_softmax(leaky_relu(el[h][idx] + er[h][row], negative_slope))      h < H
    out[r, s] = sum_{e in row r} alpha[s // F, e] * X[idx[e], s]                      F = D // H

Every per-head array is head-major (``alpha [H, E]``, ``el``, ``er`` ``[H, N]``); row ``h`` is
what the single-head entry points take, and ``alpha[h]`` is a valid ``edge_weight=``.

* :func:`gat_attention_heads` (:class:`GATAttentionHeadsFunction`): the three kernels of
  :mod:`maxk_kernels.attention` with the head as a second grid coordinate, one launch each for all
  heads.
* :func:`heads_aggregate` (:class:`HeadsAggregateFunction`): one pass over the edges weighs every
  CBSR slot by its own head's ``alpha``; the backward gathers ``grad_out`` once for both
  ``grad_sp`` and ``grad_alpha`` over the graph's cached transposed structure. No plan and no
  value refresh. :func:`maxk_heads_aggregate` puts the MaxK top-k (plain tables, with the fused
  dropout) in front and the MaxK scatter behind.
* ``torch.ops.maxk.gat_attention_heads`` and ``torch.ops.maxk.heads_aggregate`` with fake kernels
  and registered derivatives made of operators of their own.

All backwards are first order only (:func:`maxk_kernels.autograd.first_order_only`).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .autograd import CSRGraph, first_order_only, maxk

_NS = "maxk"


class GATAttentionHeadsFunction(torch.autograd.Function):
    """``alpha [H, E]`` from ``el``, ``er`` ``[H, N]`` on a CSRGraph. Saved: ``alpha``, ``el``,
    ``er``. The column pass runs only when ``el`` needs a gradient; nothing runs when neither
    input does, or when the output was not used."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, el: torch.Tensor, er: torch.Tensor, negative_slope: float):
        el, er = el.contiguous(), er.contiguous()
        alpha = ops.gat_attention_heads(graph.ptr, graph.idx, el, er, negative_slope)
        ctx.save_for_backward(alpha, el, er)
        ctx.graph = graph
        ctx.negative_slope = float(negative_slope)
        ctx.set_materialize_grads(False)  # an unused output arrives as None, not as zeros
        return alpha

    @staticmethod
    @first_order_only
    def backward(ctx, grad_alpha):
        need_el, need_er = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_alpha is None or not (need_el or need_er):
            return None, None, None, None
        alpha, el, er = ctx.saved_tensors  # read once (checkpoint unpacks per read)
        graph = ctx.graph
        grad_edge, grad_er = ops.gat_attention_backward_heads(
            graph.ptr, graph.idx, el, er, ctx.negative_slope, alpha, grad_alpha.contiguous())
        grad_el = None
        if need_el:
            grad_el = ops.edge_colsum_heads(graph.transposed_structure()[0],
                                            graph.transposed_order(), grad_edge)
        return None, grad_el, grad_er if need_er else None, None


def gat_attention_heads(graph: CSRGraph, el: torch.Tensor, er: torch.Tensor,
                        negative_slope: float = 0.2) -> torch.Tensor:
    """Attention weights ``alpha [H, E]`` of ``H``-head GAT in the CSRGraph's own edge order,
    differentiable in ``el`` and ``er`` (f32 ``[H, N]`` on the graph's device). Row ``h`` is
    :func:`maxk_kernels.gat_attention` of ``el[h]``, ``er[h]`` bit for bit."""
    for t, name in ((el, "el"), (er, "er")):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and
                t.shape[0] >= 1 and t.shape[1] == graph.num_nodes and t.device == graph.device):
            raise RuntimeError(
                f"{name} must be a float32 [num_heads, num_nodes] tensor on the graph's device")
    if el.shape != er.shape:
        raise RuntimeError("el and er must have the same number of heads")
    return GATAttentionHeadsFunction.apply(graph, el, er, float(negative_slope))


class HeadsAggregateFunction(torch.autograd.Function):
    """``out [N, D]`` from ``alpha [H, E]`` and the CBSR tables on a CSRGraph. Saved: ``alpha``,
    ``sp_data``, ``sp_index``. The backward is one kernel for both gradients; a half whose input
    needs no gradient is not computed, and nothing runs when neither does."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, alpha: torch.Tensor, sp_data: torch.Tensor,
                sp_index: torch.Tensor, dim_origin: int):
        alpha = alpha.contiguous()
        out = ops.heads_aggregate(graph.ptr, graph.idx, alpha, sp_data, sp_index, dim_origin)
        ctx.save_for_backward(alpha, sp_data, sp_index)
        ctx.graph = graph
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        need_alpha, need_sp = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_out is None or not (need_alpha or need_sp):
            return None, None, None, None, None
        alpha, sp_data, sp_index = ctx.saved_tensors  # read once
        graph = ctx.graph
        ptr_t, idx_t, _ = graph.transposed_structure()
        grad_sp, grad_alpha = ops.heads_aggregate_backward(
            ptr_t, idx_t, graph.transposed_order(), alpha, ops._rows_in_place(grad_out), sp_data,
            sp_index, need_sp=need_sp, need_alpha=need_alpha)
        return None, grad_alpha, grad_sp, None, None


def _check_alpha(graph: CSRGraph, alpha, dim_origin: int) -> None:
    if not (isinstance(alpha, torch.Tensor) and alpha.dtype == torch.float32 and
            alpha.dim() == 2 and alpha.shape[0] >= 1 and alpha.shape[1] == graph.num_edges and
            alpha.device == graph.device):
        raise RuntimeError(
            "alpha must be a float32 [num_heads, num_edges] tensor on the graph's device")
    if dim_origin > 256:
        raise RuntimeError("num_heads * out_feats = D <= 256 (u8 selectors), got "
                           f"{dim_origin}")
    if dim_origin % alpha.shape[0] != 0:
        raise RuntimeError("the number of heads must divide dim_origin")


def heads_aggregate(graph: CSRGraph, alpha: torch.Tensor, sp_data: torch.Tensor,
                    sp_index: torch.Tensor, dim_origin: int) -> torch.Tensor:
    """``out [N, D]``: every slot of ``densify(sp_data, sp_index)`` weighed by the ``alpha`` of
    its own head and summed over each row's in-edges, differentiable in ``alpha [H, E]`` and
    ``sp_data`` (HeadsAggregateFunction). The graph's edge values are not used (attention weights
    replace them, as on ``with_values("sum")``)."""
    _check_alpha(graph, alpha, int(dim_origin))
    return HeadsAggregateFunction.apply(graph, alpha, sp_data, sp_index, int(dim_origin))


def maxk_heads_aggregate(x: torch.Tensor, graph: CSRGraph, alpha: torch.Tensor, k: int,
                         mode: str = "exact", dropout_p: float = 0.0, training: bool = True,
                         seed: Optional[int] = None) -> torch.Tensor:
    """MaxK then the multi-head aggregation: ``heads_aggregate(graph, alpha, *maxk(x, k), D)``
    with the top-k writing the plain tables (``dropout_p``, ``training``, ``seed`` as for
    :func:`maxk_kernels.maxk`: the dropout inside the top-k and its scatter), differentiable in
    ``x`` and ``alpha``. The backward is the fused kernel followed by the MaxK scatter;
    ``ref_compat`` padding slots carry no gradient."""
    _check_alpha(graph, alpha, x.shape[1])
    sp_data, sp_index = maxk(x, k, mode, dropout_p=dropout_p, training=training, seed=seed)
    return HeadsAggregateFunction.apply(graph, alpha, sp_data, sp_index, x.shape[1])


# -------------------------------------------------------------------------------- operators
@torch.library.custom_op(f"{_NS}::gat_attention_heads", mutates_args=())
def gat_attention_heads_op(ptr: torch.Tensor, idx: torch.Tensor, ptr_t: torch.Tensor,
                           order: torch.Tensor, el: torch.Tensor, er: torch.Tensor,
                           negative_slope: float) -> torch.Tensor:
    """``ops.gat_attention_heads``; ``ptr_t`` and ``order`` are read by the derivative only."""
    return ops.gat_attention_heads(ptr, idx, el.contiguous(), er.contiguous(), negative_slope)


@gat_attention_heads_op.register_fake
def _(ptr, idx, ptr_t, order, el, er, negative_slope):
    return el.new_empty((el.shape[0], idx.shape[0]))


@torch.library.custom_op(f"{_NS}::gat_attention_backward_heads", mutates_args=())
def gat_attention_backward_heads_op(ptr: torch.Tensor, idx: torch.Tensor, el: torch.Tensor,
                                    er: torch.Tensor, negative_slope: float,
                                    alpha: torch.Tensor, grad_alpha: torch.Tensor
                                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(grad_edge [H, E], grad_er [H, num_rows])`` (ops.gat_attention_backward_heads)."""
    return ops.gat_attention_backward_heads(ptr, idx, el.contiguous(), er.contiguous(),
                                            negative_slope, alpha, grad_alpha)


@gat_attention_backward_heads_op.register_fake
def _(ptr, idx, el, er, negative_slope, alpha, grad_alpha):
    return alpha.new_empty(alpha.shape), er.new_empty(er.shape)


@torch.library.custom_op(f"{_NS}::edge_colsum_heads", mutates_args=())
def edge_colsum_heads_op(ptr_t: torch.Tensor, order: torch.Tensor,
                         values: torch.Tensor) -> torch.Tensor:
    """Per-head column sums ``[H, num_cols]`` (ops.edge_colsum_heads)."""
    return ops.edge_colsum_heads(ptr_t, order, values)


@edge_colsum_heads_op.register_fake
def _(ptr_t, order, values):
    return values.new_empty((values.shape[0], ptr_t.shape[0] - 1))


def _gat_heads_setup(ctx, inputs, output):
    ptr, idx, ptr_t, order, el, er, negative_slope = inputs
    ctx.save_for_backward(ptr, idx, ptr_t, order, el, er, output)
    ctx.negative_slope = negative_slope
    ctx.set_materialize_grads(False)


@first_order_only
def _gat_heads_backward(ctx, grad):
    need_el, need_er = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
    if grad is None or not (need_el or need_er):
        return (None,) * 7
    ptr, idx, ptr_t, order, el, er, alpha = ctx.saved_tensors  # read once
    grad_edge, grad_er = torch.ops.maxk.gat_attention_backward_heads(
        ptr, idx, el, er, ctx.negative_slope, alpha, grad.contiguous())
    grad_el = torch.ops.maxk.edge_colsum_heads(ptr_t, order, grad_edge) if need_el else None
    return None, None, None, None, grad_el, grad_er if need_er else None, None


gat_attention_heads_op.register_autograd(_gat_heads_backward, setup_context=_gat_heads_setup)


@torch.library.custom_op(f"{_NS}::heads_aggregate", mutates_args=())
def heads_aggregate_op(ptr: torch.Tensor, idx: torch.Tensor, ptr_t: torch.Tensor,
                       idx_t: torch.Tensor, order: torch.Tensor, alpha: torch.Tensor,
                       sp_data: torch.Tensor, sp_index: torch.Tensor,
                       dim_origin: int) -> torch.Tensor:
    """``ops.heads_aggregate``; the transposed structure ``(ptr_t, idx_t, order)``, int32, is
    read by the derivative only."""
    return ops.heads_aggregate(ptr, idx, alpha.contiguous(), sp_data, sp_index, dim_origin)


@heads_aggregate_op.register_fake
def _(ptr, idx, ptr_t, idx_t, order, alpha, sp_data, sp_index, dim_origin):
    return sp_data.new_empty((ptr.shape[0] - 1, dim_origin))


@torch.library.custom_op(f"{_NS}::heads_aggregate_backward", mutates_args=())
def heads_aggregate_backward_op(ptr_t: torch.Tensor, idx_t: torch.Tensor, order: torch.Tensor,
                                alpha: torch.Tensor, grad_out: torch.Tensor,
                                sp_data: torch.Tensor, sp_index: torch.Tensor, need_sp: bool,
                                need_alpha: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(grad_sp [num_cols, k], grad_alpha [H, E])`` (ops.heads_aggregate_backward); a half that
    is not needed comes back as an empty ``[0]`` tensor and is not computed."""
    grad_sp, grad_alpha = ops.heads_aggregate_backward(ptr_t, idx_t, order, alpha.contiguous(),
                                                       grad_out.contiguous(), sp_data, sp_index,
                                                       need_sp=need_sp, need_alpha=need_alpha)
    none = sp_data.new_empty((0,))
    return (grad_sp if need_sp else none), (grad_alpha if need_alpha else none.clone())


@heads_aggregate_backward_op.register_fake
def _(ptr_t, idx_t, order, alpha, grad_out, sp_data, sp_index, need_sp, need_alpha):
    return (sp_data.new_empty(sp_data.shape if need_sp else (0,)),
            alpha.new_empty(alpha.shape if need_alpha else (0,)))


def _heads_aggregate_setup(ctx, inputs, output):
    ptr, idx, ptr_t, idx_t, order, alpha, sp_data, sp_index, dim_origin = inputs
    ctx.save_for_backward(ptr_t, idx_t, order, alpha, sp_data, sp_index)
    ctx.set_materialize_grads(False)


@first_order_only
def _heads_aggregate_backward(ctx, grad):
    need_alpha, need_sp = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
    if grad is None or not (need_alpha or need_sp):
        return (None,) * 9
    ptr_t, idx_t, order, alpha, sp_data, sp_index = ctx.saved_tensors  # read once
    grad_sp, grad_alpha = torch.ops.maxk.heads_aggregate_backward(
        ptr_t, idx_t, order, alpha, grad, sp_data, sp_index, need_sp, need_alpha)
    return (None, None, None, None, None, grad_alpha if need_alpha else None,
            grad_sp if need_sp else None, None, None)


heads_aggregate_op.register_autograd(_heads_aggregate_backward,
                                     setup_context=_heads_aggregate_setup)
