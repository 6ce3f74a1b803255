"""Max aggregation of MaxK features: the reducer of GraphSAGE's ``pool`` aggregator.

    out[r, s] = max_{e in row r} X[idx[e], s]          X = the MaxK rows, zeros where unselected

as DGL's ``update_all(copy_u, max)`` computes it on the densified rows, by kernels that never
form the ``[E, D]`` messages (include/maxk_hip.h, "Max aggregation"). The forward records the
winner of every output element (``arg_edge``, ``arg_slot``); the backward hands each gradient
element to that one slot, where torch's ``amax`` would spread it over ties.

* :func:`max_aggregate` (:class:`MaxAggregateFunction`) on CBSR tables; :func:`maxk_max_aggregate`
  puts the MaxK top-k in front; :func:`dense_max_aggregate` runs the same kernels on dense
  features with ``k = D`` and identity selectors (the ReLU layers).
* ``torch.ops.maxk.max_aggregate`` / ``max_aggregate_backward`` with fake kernels and a
  registered derivative.

The backward is first order only (:func:`maxk_kernels.autograd.first_order_only`). No plan is
built and the graph's edge values are not used.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .autograd import CSRGraph, first_order_only, maxk

_NS = "maxk"


def _check_rows(graph: CSRGraph) -> None:
    """The forward's precondition, checked once per graph: every row is shorter than 2^24 edges
    (a graph with fewer edges than that needs no look at its rows)."""
    if graph.num_edges < ops.MAX_ROW_EDGES:
        return
    longest = graph._values.get("max_row_edges")
    if longest is None:
        longest = int(graph.in_degrees().max().item())
        graph._values["max_row_edges"] = longest
    if longest >= ops.MAX_ROW_EDGES:
        raise RuntimeError(f"max_aggregate: a row of {longest} edges; rows must be shorter than "
                           f"{ops.MAX_ROW_EDGES}")


class MaxAggregateFunction(torch.autograd.Function):
    """``(out, arg_edge, arg_slot)`` from the CBSR tables on a CSRGraph. Saved: ``arg_edge``,
    ``arg_slot``, ``sp_index``. ``with_arg=False`` (no gradient will be asked for, and the caller
    does not want the winners) runs the forward that writes ``out`` alone and returns empty
    ``arg_*``. The backward is skipped when ``sp_data`` needs no gradient."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, sp_data: torch.Tensor, sp_index: torch.Tensor,
                dim_origin: int, with_arg: bool):
        out, arg_edge, arg_slot = ops.max_aggregate_forward(
            graph.ptr, graph.idx, ops._rows_in_place(sp_data), sp_index, dim_origin, with_arg)
        if not with_arg:
            arg_edge = torch.empty((0,), dtype=torch.int32, device=out.device)
            arg_slot = torch.empty((0,), dtype=torch.uint8, device=out.device)
        ctx.save_for_backward(arg_edge, arg_slot, sp_index)
        ctx.graph = graph
        ctx.with_arg = with_arg
        ctx.mark_non_differentiable(arg_edge, arg_slot)
        ctx.set_materialize_grads(False)
        return out, arg_edge, arg_slot

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out, _grad_edge, _grad_slot):
        if grad_out is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        if not ctx.with_arg:
            raise RuntimeError("max_aggregate: the forward ran without arg_edge / arg_slot")
        arg_edge, arg_slot, sp_index = ctx.saved_tensors  # read once
        graph = ctx.graph
        ptr_t, idx_t, _ = graph.transposed_structure()
        grad_sp = ops.max_aggregate_backward(ptr_t, idx_t, graph.transposed_order(),
                                             ops._rows_in_place(grad_out), arg_edge, arg_slot,
                                             sp_index)
        return None, grad_sp, None, None, None


def _check_tables(graph: CSRGraph, sp_data, sp_index, dim_origin: int) -> None:
    if not (isinstance(sp_data, torch.Tensor) and sp_data.dtype == torch.float32 and
            sp_data.dim() == 2 and sp_data.device == graph.device):
        raise RuntimeError("sp_data must be a float32 [num_cols, k] tensor on the graph's device")
    if not (isinstance(sp_index, torch.Tensor) and sp_index.dtype == torch.uint8 and
            sp_index.shape == sp_data.shape and sp_index.device == graph.device):
        raise RuntimeError("sp_index must be a uint8 tensor of sp_data's shape on its device")
    if not 1 <= sp_data.shape[1] <= dim_origin <= 256:
        raise RuntimeError(f"1 <= k <= dim_origin <= 256 (u8 selectors), got k = "
                           f"{sp_data.shape[1]}, dim_origin = {dim_origin}")


def max_aggregate(graph: CSRGraph, sp_data: torch.Tensor, sp_index: torch.Tensor,
                  dim_origin: int, return_arg: bool = False):
    """``out [N, D]``: the maximum over each row's in-edges of the densified CBSR rows, zeros
    where a column did not select the feature (and ``+0.0`` for a row without edges),
    differentiable in ``sp_data``: each gradient element goes to the one winning slot (lowest
    edge, then lowest slot among equals), none where the implicit zero won. ``return_arg=True``
    returns ``(out, arg_edge int32, arg_slot u8)``, the winners' CSR edges (``-1``: the implicit
    zero) and slots. The graph's edge values are not used."""
    _check_tables(graph, sp_data, sp_index, int(dim_origin))
    _check_rows(graph)
    with_arg = bool(return_arg) or (torch.is_grad_enabled() and sp_data.requires_grad)
    out, arg_edge, arg_slot = MaxAggregateFunction.apply(graph, sp_data, sp_index,
                                                        int(dim_origin), with_arg)
    return (out, arg_edge, arg_slot) if return_arg else out


def maxk_max_aggregate(x: torch.Tensor, graph: CSRGraph, k: int, mode: str = "exact",
                       dropout_p: float = 0.0, training: bool = True,
                       seed: Optional[int] = None) -> torch.Tensor:
    """MaxK then the max aggregation: ``max_aggregate(graph, *maxk(x, k), D)`` with
    ``dropout_p``, ``training``, ``seed`` as for :func:`maxk_kernels.maxk`, differentiable in
    ``x`` (the max backward followed by the MaxK scatter)."""
    sp_data, sp_index = maxk(x, k, mode, dropout_p=dropout_p, training=training, seed=seed)
    return max_aggregate(graph, sp_data, sp_index, x.shape[1])


def _identity_selectors(graph: CSRGraph, rows: int, dim: int) -> torch.Tensor:
    key = ("identity_selectors", rows, dim)
    sel = graph._values.get(key)
    if sel is None:
        sel = torch.arange(dim, dtype=torch.uint8, device=graph.device).repeat(rows, 1)
        graph._values[key] = sel
    return sel


def dense_max_aggregate(x: torch.Tensor, graph: CSRGraph) -> torch.Tensor:
    """``out[r] = max_{e in row r} x[idx[e]]`` for dense ``x [N, D]``, ``D <= 256`` (DGL's
    ``copy_u`` / ``max``; ``+0.0`` for a row without edges), differentiable in ``x``: the same
    kernels with ``k = D`` and identity selectors, so every candidate is explicit."""
    if x.dim() != 2 or not 1 <= x.shape[1] <= 256:
        raise RuntimeError("dense_max_aggregate: x must be [N, D] with D <= 256")
    return max_aggregate(graph, x, _identity_selectors(graph, x.shape[0], x.shape[1]), x.shape[1])


# -------------------------------------------------------------------------------- operators
@torch.library.custom_op(f"{_NS}::max_aggregate", mutates_args=())
def max_aggregate_op(ptr: torch.Tensor, idx: torch.Tensor, ptr_t: torch.Tensor,
                     idx_t: torch.Tensor, order: torch.Tensor, sp_data: torch.Tensor,
                     sp_index: torch.Tensor, dim_origin: int
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ops.max_aggregate_forward`` with the winners; the transposed structure ``(ptr_t, idx_t,
    order)``, int32, is read by the derivative only."""
    return ops.max_aggregate_forward(ptr, idx, ops._rows_in_place(sp_data), sp_index, dim_origin,
                                     True)


@max_aggregate_op.register_fake
def _(ptr, idx, ptr_t, idx_t, order, sp_data, sp_index, dim_origin):
    shape = (ptr.shape[0] - 1, dim_origin)
    return (sp_data.new_empty(shape), idx.new_empty(shape, dtype=torch.int32),
            sp_index.new_empty(shape, dtype=torch.uint8))


@torch.library.custom_op(f"{_NS}::max_aggregate_backward", mutates_args=())
def max_aggregate_backward_op(ptr_t: torch.Tensor, idx_t: torch.Tensor, order: torch.Tensor,
                              grad_out: torch.Tensor, arg_edge: torch.Tensor,
                              arg_slot: torch.Tensor, sp_index: torch.Tensor) -> torch.Tensor:
    """``grad_sp [num_cols, k]`` (ops.max_aggregate_backward)."""
    return ops.max_aggregate_backward(ptr_t, idx_t, order, ops._rows_in_place(grad_out), arg_edge,
                                      arg_slot, sp_index)


@max_aggregate_backward_op.register_fake
def _(ptr_t, idx_t, order, grad_out, arg_edge, arg_slot, sp_index):
    return grad_out.new_empty(sp_index.shape)


def _max_aggregate_setup(ctx, inputs, output):
    ptr, idx, ptr_t, idx_t, order, sp_data, sp_index, dim_origin = inputs
    _, arg_edge, arg_slot = output
    ctx.save_for_backward(ptr_t, idx_t, order, arg_edge, arg_slot, sp_index)
    ctx.set_materialize_grads(False)


@first_order_only
def _max_aggregate_backward(ctx, grad, _grad_edge, _grad_slot):
    if grad is None or not ctx.needs_input_grad[5]:
        return (None,) * 8
    ptr_t, idx_t, order, arg_edge, arg_slot, sp_index = ctx.saved_tensors  # read once
    grad_sp = torch.ops.maxk.max_aggregate_backward(ptr_t, idx_t, order, grad, arg_edge,
                                                    arg_slot, sp_index)
    return None, None, None, None, None, grad_sp, None, None


max_aggregate_op.register_autograd(_max_aggregate_backward, setup_context=_max_aggregate_setup)
