"""The four reference entry points as registered torch operators (``torch.ops.maxk.*``).

The reference binds its kernels as a pybind11 ``CUDAExtension`` (``/root/reference/setup.py``
lines 23-24): calls are opaque to torch's tracing tools. Here the same four functions are
also registered through ``torch.library`` with shape-only fake kernels, so
``torch.compile(fullgraph=True)``, ``make_fx``/export and FakeTensor shape propagation see
one node per call instead of a graph break, and ``spgemm_forward`` carries its autograd
formula (the SSpMM backward) as a registered derivative.

    torch.ops.maxk.maxk_forward(input, k) -> (sp_data [N, k] f32, sp_index [N, k] u8)
    torch.ops.maxk.maxk_backward(grad_output, indices, dim_origin) -> [N, dim_origin]
    torch.ops.maxk.spgemm_forward(ptr, idx, val, sp_data, sp_index, num_nodes, num_edges,
                                  dim_k, dim_origin) -> out [num_nodes, dim_origin]
    torch.ops.maxk.spgemm_backward(ptr, idx, val, grad_output, sp_index, num_nodes,
                                   num_edges, dim_k, dim_origin) -> grad_sp [num_nodes, dim_k]
    torch.ops.maxk.spgemm_edge_grad(ptr, idx, grad_output, sp_data, sp_index, num_nodes,
                                    num_edges, dim_k, dim_origin) -> grad_val [num_edges]
                                  (what spgemm_forward's derivative returns for a val that
                                   requires grad)

    torch.ops.maxk.edge_softmax(ptr, logits) -> [num_edges]   (softmax over each row's in-edges,
                                  with its registered derivative)
    torch.ops.maxk.edge_softmax_backward(ptr, y, grad_y) -> grad_logits [num_edges]

    torch.ops.maxk.maxk_dropout_forward(input, k, p, seed) -> (sp_data, sp_index)
    torch.ops.maxk.maxk_dropout_backward(grad_output, indices, dim_origin, p, seed)
                                  -> [N, dim_origin]   (MaxK with fused feature dropout)

    torch.ops.maxk.maxk_dense_forward(input, k, p, seed) -> (dense [N, D], sp_data, sp_index)
    torch.ops.maxk.maxk_merge_backward(grad_output (or None), indices, grad_dense, p, seed)
                                  -> [N, D]   (MaxK that also emits the dense masked row; the
                                     scatter adds the dense row's gradient; p = 0: no dropout)

    torch.ops.maxk.csr_transpose(ptr, idx, val (or None), num_cols)
                                  -> (ptr_t [num_cols + 1], idx_t [E], order [E], val_t [E], all
                                     int32 but the f32 val_t, which is empty without val): A^T of a
                                     CSR graph; shapes from the inputs' shapes, no derivative

The real kernels are :mod:`maxk_kernels.ops` (the HIP C ABI); there is no other
implementation behind these names. Differences from the plain functions, all forced by
the operator schema: ``maxk_forward`` always returns the selectors (the reference drops
them); ``maxk_backward`` takes ``dim_origin`` (a data-dependent width has no fake shape);
``spgemm_forward`` returns ``out`` alone (an operator output may not alias the
``sp_index`` input the reference hands back).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .autograd import first_order_only

_NS = "maxk"


@torch.library.custom_op(f"{_NS}::maxk_forward", mutates_args=())
def maxk_forward(input: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxK top-k -> CBSR (ops.maxk_forward, exact mode)."""
    return ops.maxk_forward(input, k, return_index=True)


@maxk_forward.register_fake
def _(input, k):
    n = input.shape[0]
    return (input.new_empty((n, k)), input.new_empty((n, k), dtype=torch.uint8))


@torch.library.custom_op(f"{_NS}::maxk_backward", mutates_args=())
def maxk_backward(grad_output: torch.Tensor, indices: torch.Tensor,
                  dim_origin: int) -> torch.Tensor:
    """Dense MaxK gradient from the [N, k] CBSR gradient (ops.maxk_backward)."""
    return ops.maxk_backward(grad_output, indices, dim_origin)


@maxk_backward.register_fake
def _(grad_output, indices, dim_origin):
    return grad_output.new_empty((grad_output.shape[0], dim_origin))


@torch.library.custom_op(f"{_NS}::spgemm_forward", mutates_args=())
def spgemm_forward(ptr: torch.Tensor, idx: torch.Tensor, val: torch.Tensor,
                   sp_data: torch.Tensor, sp_index: torch.Tensor, num_nodes: int,
                   num_edges: int, dim_k: int, dim_origin: int) -> torch.Tensor:
    """SpGEMM forward ``out = A @ densify(sp_data, sp_index)`` (ops.spgemm_forward)."""
    return ops.spgemm_forward(ptr, idx, val, sp_data, sp_index, num_nodes, num_edges,
                              dim_k, dim_origin)[0]


@spgemm_forward.register_fake
def _(ptr, idx, val, sp_data, sp_index, num_nodes, num_edges, dim_k, dim_origin):
    return sp_data.new_empty((num_nodes, dim_origin))


@torch.library.custom_op(f"{_NS}::spgemm_backward", mutates_args=())
def spgemm_backward(ptr: torch.Tensor, idx: torch.Tensor, val: torch.Tensor,
                    grad_output: torch.Tensor, sp_index: torch.Tensor, num_nodes: int,
                    num_edges: int, dim_k: int, dim_origin: int) -> torch.Tensor:
    """SSpMM backward ``grad_sp[c, l] = sum_(r,c) val * grad_output[r, sp_index[c, l]]``."""
    return ops.spgemm_backward(ptr, idx, val, grad_output, sp_index, num_nodes, num_edges,
                               dim_k, dim_origin)


@spgemm_backward.register_fake
def _(ptr, idx, val, grad_output, sp_index, num_nodes, num_edges, dim_k, dim_origin):
    return grad_output.new_empty((num_nodes, dim_k))


@torch.library.custom_op(f"{_NS}::spgemm_edge_grad", mutates_args=())
def spgemm_edge_grad(ptr: torch.Tensor, idx: torch.Tensor, grad_output: torch.Tensor,
                     sp_data: torch.Tensor, sp_index: torch.Tensor, num_nodes: int,
                     num_edges: int, dim_k: int, dim_origin: int) -> torch.Tensor:
    """SDDMM ``grad_val[e] = sum_l sp_data[c, l] * grad_output[r, sp_index[c, l]]``, the
    gradient of ``spgemm_forward`` with respect to ``val`` (ops.spgemm_edge_grad)."""
    return ops.spgemm_edge_grad(ptr, idx, grad_output, sp_data, sp_index, num_nodes, num_edges,
                                dim_k, dim_origin)


@spgemm_edge_grad.register_fake
def _(ptr, idx, grad_output, sp_data, sp_index, num_nodes, num_edges, dim_k, dim_origin):
    return grad_output.new_empty((num_edges,))


def _spgemm_setup(ctx, inputs, output):
    ptr, idx, val, sp_data, sp_index, num_nodes, num_edges, dim_k, dim_origin = inputs
    # the value table is saved only for a val that needs a gradient
    ctx.save_for_backward(ptr, idx, val, sp_index, *((sp_data,) if ctx.needs_input_grad[2] else ()))
    ctx.dims = (num_nodes, num_edges, dim_k, dim_origin)


@first_order_only
def _spgemm_backward(ctx, grad):
    saved = ctx.saved_tensors  # read once (checkpoint unpacks per read)
    ptr, idx, val, sp_index = saved[:4]
    grad = grad.contiguous()
    grad_sp = grad_val = None
    if ctx.needs_input_grad[3]:  # no SSpMM for a constant table (only val needs a gradient)
        grad_sp = torch.ops.maxk.spgemm_backward(ptr, idx, val, grad, sp_index, *ctx.dims)
    if ctx.needs_input_grad[2]:
        grad_val = torch.ops.maxk.spgemm_edge_grad(ptr, idx, grad, saved[4], sp_index,
                                                   *ctx.dims)
    return None, None, grad_val, grad_sp, None, None, None, None, None


spgemm_forward.register_autograd(_spgemm_backward, setup_context=_spgemm_setup)


@torch.library.custom_op(f"{_NS}::edge_softmax", mutates_args=())
def edge_softmax(ptr: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """Softmax of per-edge logits over each destination row's in-edges (ops.edge_softmax)."""
    return ops.edge_softmax(ptr, logits)


@edge_softmax.register_fake
def _(ptr, logits):
    return logits.new_empty(logits.shape)


@torch.library.custom_op(f"{_NS}::edge_softmax_backward", mutates_args=())
def edge_softmax_backward(ptr: torch.Tensor, y: torch.Tensor,
                          grad_y: torch.Tensor) -> torch.Tensor:
    """``y * (grad_y - sum_row(y * grad_y))``, the gradient of ``edge_softmax`` from its output
    (ops.edge_softmax_backward)."""
    return ops.edge_softmax_backward(ptr, y, grad_y)


@edge_softmax_backward.register_fake
def _(ptr, y, grad_y):
    return y.new_empty(y.shape)


def _edge_softmax_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output)  # the output only: the backward reads no logits


@first_order_only
def _edge_softmax_backward(ctx, grad):
    ptr, y = ctx.saved_tensors
    return None, torch.ops.maxk.edge_softmax_backward(ptr, y, grad.contiguous())


edge_softmax.register_autograd(_edge_softmax_backward, setup_context=_edge_softmax_setup)


def _maxk_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.dim_origin = inputs[0].shape[1]


@first_order_only
def _maxk_backward(ctx, grad_data, grad_index):
    (sp_index,) = ctx.saved_tensors
    if grad_data is None:
        return None, None
    return torch.ops.maxk.maxk_backward(grad_data.contiguous(), sp_index, ctx.dim_origin), None


maxk_forward.register_autograd(_maxk_backward, setup_context=_maxk_setup)


# MaxK with fused feature dropout (ops.maxk_forward / ops.maxk_backward ``dropout=``). ``seed``
# is an int64 schema int, reinterpreted as the uint64 seed of the mask.
@torch.library.custom_op(f"{_NS}::maxk_dropout_forward", mutates_args=())
def maxk_dropout_forward(input: torch.Tensor, k: int, p: float,
                         seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxK top-k -> CBSR with dropout on the kept values (exact mode)."""
    return ops.maxk_forward(input, k, return_index=True, dropout=(p, seed))


@maxk_dropout_forward.register_fake
def _(input, k, p, seed):
    n = input.shape[0]
    return (input.new_empty((n, k)), input.new_empty((n, k), dtype=torch.uint8))


@torch.library.custom_op(f"{_NS}::maxk_dropout_backward", mutates_args=())
def maxk_dropout_backward(grad_output: torch.Tensor, indices: torch.Tensor, dim_origin: int,
                          p: float, seed: int) -> torch.Tensor:
    """Dense MaxK gradient through the same dropout mask (ops.maxk_backward ``dropout=``)."""
    return ops.maxk_backward(grad_output, indices, dim_origin, dropout=(p, seed))


@maxk_dropout_backward.register_fake
def _(grad_output, indices, dim_origin, p, seed):
    return grad_output.new_empty((grad_output.shape[0], dim_origin))


def _maxk_dropout_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.dim_origin = inputs[0].shape[1]
    ctx.dropout = (inputs[2], inputs[3])


@first_order_only
def _maxk_dropout_backward(ctx, grad_data, grad_index):
    (sp_index,) = ctx.saved_tensors
    if grad_data is None:
        return None, None, None, None
    return (torch.ops.maxk.maxk_dropout_backward(grad_data.contiguous(), sp_index,
                                                 ctx.dim_origin, *ctx.dropout),
            None, None, None)


maxk_dropout_forward.register_autograd(_maxk_dropout_backward,
                                       setup_context=_maxk_dropout_setup)


# MaxK that also emits the dense masked row (ops.maxk_forward ``dense=``) and the scatter that
# merges the two outputs' gradients (ops.maxk_backward ``grad_dense=``); ``p == 0``: no dropout.
@torch.library.custom_op(f"{_NS}::maxk_dense_forward", mutates_args=())
def maxk_dense_forward(input: torch.Tensor, k: int, p: float,
                       seed: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """MaxK top-k -> (dense masked row, CBSR values, selectors), exact mode."""
    dense = torch.empty_like(input, memory_format=torch.contiguous_format)
    sp_data, sp_index = ops.maxk_forward(input, k, return_index=True, dropout=(p, seed),
                                         dense=dense)
    return dense, sp_data, sp_index


@maxk_dense_forward.register_fake
def _(input, k, p, seed):
    n = input.shape[0]
    return (input.new_empty(input.shape), input.new_empty((n, k)),
            input.new_empty((n, k), dtype=torch.uint8))


@torch.library.custom_op(f"{_NS}::maxk_merge_backward", mutates_args=())
def maxk_merge_backward(grad_output: Optional[torch.Tensor], indices: torch.Tensor,
                        grad_dense: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """Dense MaxK gradient of both outputs of ``maxk_dense_forward`` (the width is
    ``grad_dense``'s); ``grad_output=None``: only the dense output was used."""
    return ops.maxk_backward(grad_output, indices, grad_dense.shape[1], dropout=(p, seed),
                             grad_dense=grad_dense)


@maxk_merge_backward.register_fake
def _(grad_output, indices, grad_dense, p, seed):
    return grad_dense.new_empty(grad_dense.shape)


def _maxk_dense_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])
    ctx.shape = tuple(inputs[0].shape)
    ctx.dropout = (inputs[2], inputs[3])
    ctx.set_materialize_grads(False)  # an unused output arrives as None, not as zeros


@first_order_only
def _maxk_dense_backward(ctx, grad_dense, grad_data, grad_index):
    (sp_index,) = ctx.saved_tensors
    if grad_dense is None and grad_data is None:
        return None, None, None, None
    if grad_dense is None:
        return (torch.ops.maxk.maxk_dropout_backward(grad_data.contiguous(), sp_index,
                                                     ctx.shape[1], *ctx.dropout),
                None, None, None)
    if grad_data is not None:
        grad_data = grad_data.contiguous()
    return (torch.ops.maxk.maxk_merge_backward(grad_data, sp_index, grad_dense.contiguous(),
                                               *ctx.dropout),
            None, None, None)


maxk_dense_forward.register_autograd(_maxk_dense_backward, setup_context=_maxk_dense_setup)


# A^T of a CSR graph (ops.csr_transpose). The output shapes follow from the input shapes and
# num_cols alone, so it has a fake kernel; structure has no derivative.
@torch.library.custom_op(f"{_NS}::csr_transpose", mutates_args=())
def csr_transpose(ptr: torch.Tensor, idx: torch.Tensor, val: Optional[torch.Tensor],
                  num_cols: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ptr_t, idx_t, order, val_t)``; ``val_t`` has no elements when ``val`` is ``None``."""
    out = ops.csr_transpose(ptr, idx, val, num_cols)
    if val is None:
        out += (torch.empty(0, dtype=torch.float32, device=ptr.device),)
    return out


@csr_transpose.register_fake
def _(ptr, idx, val, num_cols):
    e = idx.shape[0]
    return (idx.new_empty((num_cols + 1,)), idx.new_empty((e,)), idx.new_empty((e,)),
            idx.new_empty((e if val is not None else 0,), dtype=torch.float32))
