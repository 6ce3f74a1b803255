"""The weight products on either side of a MaxK, on the CBSR tables instead of dense rows.

A node keeps ``k`` of ``D`` features, so a linear layer that reads the MaxK output, and the
backward of one that feeds it, are products of ``N k M`` multiply-adds, where the dense GEMMs on
the masked rows are ``N D M`` on operands that are ``1 - k / D`` zeros. The three kernels are
``ops.cbsr_matmul`` (A), ``ops.cbsr_sampled_matmul`` (B) and ``ops.cbsr_weight_grad`` (C)
(include/maxk_hip.h, "MaxK linear layers"):

* :func:`cbsr_linear` is ``densify(sp) @ weight.T + bias`` without the dense row: forward (A),
  backward (B) for the kept values and (C) for the weight.
* :func:`linear_maxk` is ``maxk(F.linear(h, weight, bias), k)`` whose backward takes the gradient
  of the kept values as it is: ``grad_h`` by (A) with ``weight`` as the table, ``grad_weight`` and
  ``grad_bias`` by (C) with ``h`` in the place of the gradient. No ``[N, D]`` gradient is written.
  With ``fused=True`` the forward is ``ops.linear_topk``, one launch that keeps the ``[N, D]``
  pre-activation in matrix-core accumulators, so that tensor is not written either; with bf16 or
  f16 ``h`` and ``weight`` it is the 16-bit kernel, and the backward upcasts, unless
  ``weight_grad_16=True`` hands the weight and bias gradient to ``ops.cbsr_weight_grad_16``, which
  reads the 16-bit ``h`` as it is on the matrix cores, and ``input_grad_16=True`` the input
  gradient to ``ops.cbsr_matmul_16``, which reads the 16-bit ``weight`` as it is there.

Both are first order only, as every Function of :mod:`maxk_kernels.autograd`.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ops
from .autograd import first_order_only


class CBSRMatmulFunction(torch.autograd.Function):
    """``(sp_data, sp_index, table [D, M], bias) -> densify(sp) @ table + bias``."""

    @staticmethod
    def forward(ctx, sp_data, sp_index, table, bias):
        sp_data, table = ops._rows_in_place(sp_data), ops._rows_in_place(table)
        ctx.save_for_backward(sp_data, sp_index, table)
        return ops.cbsr_matmul(sp_data, sp_index, table,
                               None if bias is None else bias.contiguous())

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        sp_data, sp_index, table = ctx.saved_tensors
        g = ops._rows_in_place(grad_out)
        need = ctx.needs_input_grad
        grad_data = ops.cbsr_sampled_matmul(g, sp_index, table) if need[0] else None
        grad_table = (ops.cbsr_weight_grad(sp_data, sp_index, g, table.shape[0])
                      if need[2] else None)
        return grad_data, None, grad_table, g.sum(0) if need[3] else None


def cbsr_linear(sp_data: torch.Tensor, sp_index: torch.Tensor, weight: torch.Tensor,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``densify(sp_data, sp_index, D) @ weight.T + bias`` as ``[N, M]`` for ``weight [M, D]``
    (``nn.Linear``'s layout), differentiable in ``sp_data``, ``weight`` and ``bias``. The table of
    the kernels is ``weight.t()`` made contiguous by torch, ``[D, M]`` (at most 256 KB)."""
    return CBSRMatmulFunction.apply(sp_data, sp_index, weight.t().contiguous(), bias)


class LinearMaxKFunction(torch.autograd.Function):
    """``(h, weight [D, D_in], bias) -> maxk(h @ weight.T + bias, k)`` in exact mode; only ``h``
    and the selectors are saved. ``fused``: the forward is ``ops.linear_topk`` instead of
    ``F.linear`` and ``ops.maxk_forward``; the backward is the same. 16-bit ``h`` and ``weight``
    (``fused`` only): ``sp_data`` is f32, the backward runs the f32 kernels on upcast copies of
    ``weight`` and ``h`` and returns every gradient in its input's dtype; ``weight_grad_16``: the
    weight and bias gradient come from ``ops.cbsr_weight_grad_16`` on ``h`` as it is;
    ``input_grad_16``: ``grad_h`` comes from ``ops.cbsr_matmul_16`` on ``weight`` as it is."""

    @staticmethod
    def forward(ctx, h, weight, bias, k, fused=False, weight_grad_16=False, input_grad_16=False):
        if fused:
            sp_data, sp_index = ops.linear_topk(
                ops._rows_in_place(h), ops._rows_in_place(weight),
                None if bias is None else bias.contiguous(), k)
        else:
            sp_data, sp_index = ops.maxk_forward(F.linear(h, weight, bias), k, mode="exact",
                                                 return_index=True)
        ctx.save_for_backward(h, weight, sp_index)
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.weight_grad_16 = weight_grad_16
        ctx.input_grad_16 = input_grad_16
        ctx.mark_non_differentiable(sp_index)
        return sp_data, sp_index

    @staticmethod
    @first_order_only
    def backward(ctx, grad_data, grad_index):
        h, weight, sp_index = ctx.saved_tensors
        grad_data = ops._rows_in_place(grad_data)
        need = ctx.needs_input_grad
        grad_h = grad_w = grad_b = None
        if need[0]:
            if ctx.input_grad_16:  # no f32 copy of weight, no f32 [N, D_in], no cast pass
                grad_h = ops.cbsr_matmul_16(grad_data, sp_index, ops._rows_in_place(weight))
            else:
                grad_h = ops.cbsr_matmul(grad_data, sp_index, ops._rows_in_place(weight.float()))
        if need[1] or need[2]:
            if ctx.weight_grad_16:  # no f32 copy of h: both operands go to the matrix cores
                res = ops.cbsr_weight_grad_16(grad_data, sp_index, ops._rows_in_place(h),
                                              weight.shape[0], with_sum=bool(need[2]))
            else:
                res = ops.cbsr_weight_grad(grad_data, sp_index, ops._rows_in_place(h.float()),
                                           weight.shape[0], with_sum=bool(need[2]))
            grad_w, grad_b = res if need[2] else (res, None)
        if h.dtype != torch.float32:  # 16-bit inputs: one rounding of each f32 gradient
            grad_h = None if grad_h is None else grad_h.to(h.dtype)
            grad_w = None if grad_w is None else grad_w.to(weight.dtype)
            grad_b = None if grad_b is None else grad_b.to(ctx.bias_dtype)
        return grad_h, grad_w if need[1] else None, grad_b, None, None, None, None


def linear_maxk(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], k: int,
                mode: str = "exact", fused: bool = False, weight_grad_16: bool = False,
                input_grad_16: bool = False):
    """``(sp_data, sp_index) = maxk(F.linear(h, weight, bias), k)`` for ``weight [D, D_in]``,
    differentiable in ``h``, ``weight`` and ``bias``. ``mode="ref_compat"`` is refused: its padding
    slots carry no gradient, which takes the rule of the scatter (``autograd._mask_padding``).
    ``fused=True`` computes the forward with ``ops.linear_topk`` (f32, ``D <= 256``): the same
    selection rules on a pre-activation whose sum over ``D_in`` runs in the matrix cores' order, so
    values agree with the default within rounding, and bit for bit on exactly summable inputs.

    The call follows the dtype of ``h`` and ``weight``. Both bf16 or both f16 needs ``fused=True``:
    the forward is the 16-bit kernel of ``ops.linear_topk`` (f32 sums, ``sp_data`` f32). Every
    gradient is computed in f32 and rounded once, ``grad_h`` and ``grad_weight`` to the inputs'
    dtype and ``grad_bias`` to the bias's. ``grad_h`` is the f32 ``cbsr_matmul`` on an f32 copy of
    ``weight``. ``grad_weight`` and ``grad_bias`` are, by default, the f32 ``cbsr_weight_grad`` on
    an f32 copy of ``h`` (``[N, D_in]``, twice the bytes of ``h``). ``weight_grad_16=True`` (16-bit
    inputs only, else ``ValueError``) computes them with ``ops.cbsr_weight_grad_16`` from ``h`` as
    it is: no copy of ``h``, both operands on the matrix cores, a fixed summation order, so the
    step repeats bit for bit. Its price is one more rounding: the gradient of each kept value is
    rounded to the inputs' dtype before it is multiplied with ``h`` (the products are then exact in
    f32 and the f32 sum keeps ``(n + 2) 2^-24 sum |terms|`` against the exact sum over the rounded
    values), where the default multiplies the f32 gradient. ``input_grad_16=True`` (16-bit inputs
    only, else ``ValueError``) does the same for ``grad_h``: ``ops.cbsr_matmul_16`` on ``weight`` as
    it is returns it in the inputs' dtype, the f32 sum of exact products rounded once, with no f32
    copy of ``weight``, no f32 ``[N, D_in]`` and no cast pass, at the same price of one rounding
    of the gradient of each kept value."""
    if mode != "exact":
        raise ValueError(f'linear_maxk supports mode="exact" only, got {mode!r}: the padding '
                         "slots of ref_compat need the MaxK scatter's rule")
    if not fused and (h.dtype in ops.LINEAR_TOPK_DTYPES or weight.dtype in ops.LINEAR_TOPK_DTYPES):
        raise ValueError(f"linear_maxk on {h.dtype} / {weight.dtype} inputs needs fused=True: only "
                         "the fused forward has a 16-bit kernel")
    if weight_grad_16 and h.dtype not in ops.LINEAR_TOPK_DTYPES:
        raise ValueError(f"weight_grad_16=True needs bfloat16 or float16 inputs, got {h.dtype}: "
                         "the f32 weight gradient is ops.cbsr_weight_grad")
    if input_grad_16 and h.dtype not in ops.LINEAR_TOPK_DTYPES:
        raise ValueError(f"input_grad_16=True needs bfloat16 or float16 inputs, got {h.dtype}: "
                         "the f32 input gradient is ops.cbsr_matmul")
    return LinearMaxKFunction.apply(h, weight, bias, k, bool(fused), bool(weight_grad_16),
                                    bool(input_grad_16))
