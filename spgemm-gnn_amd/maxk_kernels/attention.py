"""Fused single-head GAT attention: node scores to attention weights in one kernel.

    alpha = edge_softmax(leaky_relu(el[idx] + er[row], negative_slope))

``ops.gat_attention`` computes ``alpha`` from the two ``[N]`` score vectors with no ``[E]``
intermediate, bit for bit what the composition above gives through :func:`edge_softmax`. The
backward is ``ops.gat_attention_backward`` (the per-edge gradient of the score sum and its row
sums, ``grad_er``) and ``ops.edge_colsum`` over the graph's transposed structure (``grad_el``):
two kernels, no atomics, every sum in a fixed order (include/maxk_hip.h, "GAT attention").
Between forward and backward only ``alpha`` is kept (the aggregation that consumes it keeps it
anyway) beside the two inputs; the score is recomputed.

* :class:`GATAttentionFunction` / :func:`gat_attention` on a :class:`CSRGraph`;
* ``torch.ops.maxk.gat_attention(ptr, idx, ptr_t, order, el, er, negative_slope)`` with a fake
  kernel and a registered derivative, and the two operators its derivative is made of,
  ``torch.ops.maxk.gat_attention_backward`` and ``torch.ops.maxk.edge_colsum``.

The backward is first order only (:func:`maxk_kernels.autograd.first_order_only`).
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import ops
from .autograd import CSRGraph, first_order_only

_NS = "maxk"


class GATAttentionFunction(torch.autograd.Function):
    """``alpha [E]`` from ``el [N]`` (source side) and ``er [N]`` (destination side) on a
    CSRGraph. Saved: ``alpha``, ``el``, ``er``. The column pass (and the int32 transposed order it
    needs, built on first use) runs only when ``el`` needs a gradient; nothing runs when neither
    input does, or when the output was not used."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, el: torch.Tensor, er: torch.Tensor, negative_slope: float):
        el, er = el.contiguous(), er.contiguous()
        alpha = ops.gat_attention(graph.ptr, graph.idx, el, er, negative_slope)
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
        grad_edge, grad_er = ops.gat_attention_backward(graph.ptr, graph.idx, el, er,
                                                        ctx.negative_slope, alpha,
                                                        grad_alpha.contiguous())
        grad_el = None
        if need_el:
            grad_el = ops.edge_colsum(graph.transposed_structure()[0], graph.transposed_order(),
                                      grad_edge)
        return None, grad_el, grad_er if need_er else None, None


def gat_attention(graph: CSRGraph, el: torch.Tensor, er: torch.Tensor,
                  negative_slope: float = 0.2) -> torch.Tensor:
    """Attention weights ``alpha [E]`` of single-head GAT in the CSRGraph's own edge order,
    differentiable in ``el`` and ``er`` (f32 ``[N]`` on the graph's device):
    ``edge_softmax(graph, leaky_relu(el[graph.idx] + er[graph.edge_rows()], negative_slope))``
    bit for bit, from one kernel and with no ``[E]`` intermediate (GATAttentionFunction). The
    result is an ``edge_weight=`` of the aggregations."""
    for t, name in ((el, "el"), (er, "er")):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and
                t.shape == (graph.num_nodes,) and t.device == graph.device):
            raise RuntimeError(f"{name} must be a float32 [num_nodes] tensor on the graph's device")
    return GATAttentionFunction.apply(graph, el, er, float(negative_slope))


# -------------------------------------------------------------------------------- operators
@torch.library.custom_op(f"{_NS}::gat_attention", mutates_args=())
def gat_attention_op(ptr: torch.Tensor, idx: torch.Tensor, ptr_t: torch.Tensor,
                     order: torch.Tensor, el: torch.Tensor, er: torch.Tensor,
                     negative_slope: float) -> torch.Tensor:
    """``ops.gat_attention``; ``ptr_t`` and ``order`` (the transposed structure, int32) are read
    by the derivative only."""
    return ops.gat_attention(ptr, idx, el, er, negative_slope)


@gat_attention_op.register_fake
def _(ptr, idx, ptr_t, order, el, er, negative_slope):
    return el.new_empty(idx.shape)


@torch.library.custom_op(f"{_NS}::gat_attention_backward", mutates_args=())
def gat_attention_backward_op(ptr: torch.Tensor, idx: torch.Tensor, el: torch.Tensor,
                              er: torch.Tensor, negative_slope: float, alpha: torch.Tensor,
                              grad_alpha: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(grad_edge [E], grad_er [num_rows])`` (ops.gat_attention_backward)."""
    return ops.gat_attention_backward(ptr, idx, el, er, negative_slope, alpha, grad_alpha)


@gat_attention_backward_op.register_fake
def _(ptr, idx, el, er, negative_slope, alpha, grad_alpha):
    return alpha.new_empty(alpha.shape), er.new_empty(er.shape)


@torch.library.custom_op(f"{_NS}::edge_colsum", mutates_args=())
def edge_colsum_op(ptr_t: torch.Tensor, order: torch.Tensor,
                   values: torch.Tensor) -> torch.Tensor:
    """Per-column sums ``[num_cols]`` of per-edge values (ops.edge_colsum)."""
    return ops.edge_colsum(ptr_t, order, values)


@edge_colsum_op.register_fake
def _(ptr_t, order, values):
    return values.new_empty((ptr_t.shape[0] - 1,))


def _gat_attention_setup(ctx, inputs, output):
    ptr, idx, ptr_t, order, el, er, negative_slope = inputs
    ctx.save_for_backward(ptr, idx, ptr_t, order, el, er, output)
    ctx.negative_slope = negative_slope
    ctx.set_materialize_grads(False)  # an unused output arrives as None, not as zeros


@first_order_only
def _gat_attention_backward(ctx, grad):
    none = (None,) * 7
    need_el, need_er = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
    if grad is None or not (need_el or need_er):
        return none
    ptr, idx, ptr_t, order, el, er, alpha = ctx.saved_tensors  # read once
    grad_edge, grad_er = torch.ops.maxk.gat_attention_backward(
        ptr, idx, el, er, ctx.negative_slope, alpha, grad.contiguous())
    grad_el = torch.ops.maxk.edge_colsum(ptr_t, order, grad_edge) if need_el else None
    return None, None, None, None, grad_el, grad_er if need_er else None, None


gat_attention_op.register_autograd(_gat_attention_backward, setup_context=_gat_attention_setup)
