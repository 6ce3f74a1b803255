"""autograd surface for the MaxK aggregation path.

The reference has no autograd op pairing ``spgemm_forward`` with ``spgemm_backward``
(the intended pairing is sketched in newmodel.py:60-148 against a
module that does not exist) and its ``MaxKFunction`` (utils/maxk_layers.py:16-45) mixes
``[N, k]`` and dense shapes. Here:

* :class:`MaxKFunction` maps dense ``x [N, D]`` to CBSR ``(sp_data [N, k], sp_index)``;
  its backward is the device scatter ``maxk_backward`` (dense ``[N, D]``), i.e. the
  ``grad * mask`` of utils/models.py:23-26 without materialising the mask.
* :class:`SpGEMMFunction` maps CBSR features to ``Y = A @ densify(sp)`` (SpGEMM forward)
  and back-propagates with the SSpMM kernel, ``grad_sp = (A^T G)`` sampled at the
  selector.
* :class:`MaxKAggregateFunction` and :class:`MaxKSelfAggregateFunction` fuse the two, and
  :class:`EdgeWeightedFunction` does so with changing edge values. All three run one forward,
  :func:`_fused_forward` (the top-k writing what the plan's forward gathers, then that
  forward), and one input gradient, :func:`_maxk_input_grad` (padding, the merge of the dense
  row's gradient, the scatter), which is also the whole backward of :class:`MaxKFunction`. A
  Function picks the plan, records on ``ctx``, and in the backward checks or refreshes the edge
  values before the SSpMM.
* :class:`EdgeWeightedFunction` is the aggregation with the edge values as a differentiable
  input (``edge_weight=`` on :func:`spgemm`, :func:`maxk_aggregate`,
  :func:`maxk_self_aggregate`): the same kernels on a value-refreshed plan, plus the SDDMM
  ``ops.spgemm_edge_grad`` for the values' gradient.
* :class:`EdgeSoftmaxFunction` (:func:`edge_softmax`) normalises per-edge logits over each
  destination row's in-edges: the attention weights that ``edge_weight=`` then takes.

Every backward is first order only (:func:`first_order_only`): under ``create_graph=True`` the
gradients are the usual ones and differentiating them raises. The unweighted aggregations read
``graph.val`` again in the backward, so they remember its version and refuse a backward after an
in-place edit of it (``_check_values_version``).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import ops


def first_order_only(backward):
    """``once_differentiable`` for a backward whose body is kernel launches into fresh buffers,
    which autograd cannot see through. Under ``create_graph=True`` the returned gradients carry
    a node that raises when anything built from them is differentiated. ``once_differentiable``
    alone attaches that node only when an incoming gradient requires grad; with a constant one
    (``y.sum()``) it would hand back plain constants, and a gradient-penalty term built from them
    would drop out of the second backward without an error. Here the node is attached whenever
    the backward runs in grad mode, i.e. whenever a graph of it was asked for."""
    once = once_differentiable(backward)

    @functools.wraps(backward)
    def wrapper(ctx, *grads):
        if torch.is_grad_enabled() and not any(
                isinstance(g, torch.Tensor) and g.requires_grad for g in grads):
            grads = list(grads)
            for i, g in enumerate(grads):
                if isinstance(g, torch.Tensor) and g.is_floating_point():
                    grads[i] = g.detach().requires_grad_(True)
                    break
        return once(ctx, *grads)

    return wrapper


def _save_values_version(ctx, val: torch.Tensor) -> None:
    """The backward of an unweighted aggregation computes with ``graph.val`` again (through the
    plan's snapshot, or A^T built from it): remember which version the forward ran with."""
    ctx.val_ref, ctx.val_version = val, ops._version(val)


def _check_values_version(ctx) -> None:
    """Refuse a backward whose forward ran with other edge values: ``graph.val`` was edited in
    place since (torch's wording for a saved tensor), whether or not a later forward on the same
    graph has already refreshed the shared plan to the new values. A view of ``graph.val``
    shares its version counter, so an edit through one is seen too."""
    val = ctx.val_ref
    if ops._version(val) != ctx.val_version:
        raise RuntimeError(
            "maxk_kernels: the graph's edge values (graph.val) needed for gradient computation "
            f"have been modified by an inplace operation: they are at version {val._version}, "
            f"the forward ran with version {ctx.val_version}. Run the backward before editing "
            "graph.val, or pass the changing values as edge_weight=")


def _torch_transpose(ptr, idx, num_cols: int, rows=None):
    """``(ptr_t int64 [num_cols + 1], rows int64 [E], order int64 [E])``: the transposition in
    torch, a stable argsort of the int64 key ``column * num_rows + row``. The path of CPU tensors;
    on the GPU ``ops.csr_transpose`` computes the same (tests/test_gpu_transpose.py,
    tools/transpose_time.py). ``rows``: the row of every edge, when the caller has it."""
    n = ptr.numel() - 1
    if rows is None:
        rows = torch.repeat_interleave(torch.arange(n, device=ptr.device),
                                       (ptr[1:] - ptr[:-1]).to(torch.int64),
                                       output_size=idx.numel())
    cols = idx.to(torch.int64)
    order = torch.argsort(cols * max(n, 1) + rows, stable=True)
    ptr_t = torch.zeros(num_cols + 1, dtype=torch.int64, device=ptr.device)
    ptr_t[1:] = torch.cumsum(torch.bincount(cols, minlength=num_cols), 0)
    return ptr_t, rows, order


@dataclass
class CSRGraph:
    """Destination-row CSR adjacency: row r aggregates from columns idx[ptr[r]:ptr[r+1]].

    This is ``A`` in ``Y = A X``; for DGL's ``update_all(copy_u, ...)`` it is the CSR of
    the in-edges (row = destination node), i.e. ``g.adj_tensors('csc')`` of a DGL graph.
    (The reference takes ``adj_tensors('csr')``, the out-edge CSR, at
    utils/maxk_layers.py:106 — correct only for symmetric graphs; SURVEY §8(b) defect 5.)
    """

    ptr: torch.Tensor
    idx: torch.Tensor
    val: Optional[torch.Tensor] = None
    _values: dict = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        self.ptr = self.ptr.to(torch.int32).contiguous()
        self.idx = self.idx.to(torch.int32).contiguous()
        if self.val is None:
            self.val = torch.ones(self.idx.numel(), dtype=torch.float32, device=self.idx.device)
        self.val = self.val.to(torch.float32).contiguous()

    @property
    def num_nodes(self) -> int:
        return self.ptr.numel() - 1

    @property
    def num_edges(self) -> int:
        return self.idx.numel()

    @property
    def device(self) -> torch.device:
        return self.ptr.device

    def plan(self, dim_origin: int, dim_k: int) -> ops.GraphPlan:
        return ops.get_plan(self.ptr, self.idx, self.val, self.num_nodes, self.num_edges,
                            dim_origin, dim_k)

    def weighted_plan(self, dim_origin: int, dim_k: int) -> ops.GraphPlan:
        """The plan for edge values that change from call to call (``edge_weight=``): cached on
        this graph per (D, k), apart from :meth:`plan`, built once and from then on only
        value-refreshed (``GraphPlan.refresh_values``) to each call's effective values."""
        key = ("weighted_plan", int(dim_origin), int(dim_k))
        plan = self._values.get(key)
        if plan is None:
            plan = ops.GraphPlan(self.ptr, self.idx, self.val, self.num_nodes, self.num_edges,
                                 int(dim_origin), int(dim_k))
            self._values[key] = plan
        return plan

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_edges(cls, src: torch.Tensor, dst: torch.Tensor, num_nodes: int,
                   val: Optional[torch.Tensor] = None) -> "CSRGraph":
        """Edges u -> v (messages flow src -> dst), grouped by destination row."""
        src, dst = src.to(torch.int64), dst.to(torch.int64)
        key = dst * num_nodes + src
        order = torch.argsort(key, stable=True)
        cnt = torch.bincount(dst, minlength=num_nodes)
        ptr = torch.zeros(num_nodes + 1, dtype=torch.int64, device=src.device)
        ptr[1:] = torch.cumsum(cnt, 0)
        return cls(ptr, src[order], None if val is None else val[order])

    @classmethod
    def from_dgl(cls, g) -> "CSRGraph":
        """In-edge CSR of a homogeneous DGL graph (``adj_tensors('csc')``: indptr over
        destinations, indices = sources). Cached on the graph object."""
        cached = getattr(g, "_maxk_csr", None)
        if isinstance(cached, CSRGraph):
            return cached
        indptr, indices, _ = g.adj_tensors("csc")
        csr = cls(indptr, indices)
        try:
            g._maxk_csr = csr
        except AttributeError:  # pragma: no cover - frozen graph objects
            pass
        return csr

    # -- degrees and edge weights -----------------------------------------------------
    def in_degrees(self) -> torch.Tensor:
        return (self.ptr[1:] - self.ptr[:-1]).to(torch.int64)

    def out_degrees(self) -> torch.Tensor:
        st = self._values.get("transposed_structure")
        if st is not None:      # the column counts are the row lengths of A^T
            return (st[0][1:] - st[0][:-1]).to(torch.int64)
        return torch.bincount(self.idx.to(torch.int64), minlength=self._num_cols())

    def edge_rows(self) -> torch.Tensor:
        """The destination row of every edge, int64 ``[E]`` in CSR edge order (cached): the
        row-side gather index of a per-edge score such as ``er[edge_rows]``."""
        rows = self._values.get("edge_rows")
        if rows is None:
            rows = torch.repeat_interleave(torch.arange(self.num_nodes, device=self.device),
                                           self.in_degrees(), output_size=self.num_edges)
            self._values["edge_rows"] = rows
        return rows

    def edge_values(self, kind: str) -> torch.Tensor:
        """Per-edge weights for the aggregation ``kind`` (cached):

        * ``"sum"`` / ``"none"``: 1
        * ``"mean"`` / ``"right"``: 1 / in_deg(dst)   (DGL fn.mean, GraphConv norm='right')
        * ``"left"``: 1 / out_deg(src)
        * ``"both"``: out_deg(src)^-1/2 * in_deg(dst)^-1/2   (GraphConv norm='both')

        Degrees are clamped to >= 1 (utils/maxk_layers.py:148,302,371).
        """
        v = self._values.get(kind)
        if v is not None:
            return v
        rows = torch.repeat_interleave(torch.arange(self.num_nodes, device=self.device),
                                       self.in_degrees())
        cols = self.idx.to(torch.int64)
        ind = self.in_degrees().clamp(min=1).to(torch.float32)
        outd = self.out_degrees().clamp(min=1).to(torch.float32)
        if kind in ("sum", "none"):
            v = torch.ones(self.num_edges, dtype=torch.float32, device=self.device)
        elif kind in ("mean", "right"):
            v = (1.0 / ind)[rows]
        elif kind == "left":
            v = (1.0 / outd)[cols]
        elif kind == "both":
            v = outd.rsqrt()[cols] * ind.rsqrt()[rows]
        else:
            raise ValueError(f"unknown aggregation weights {kind!r}")
        v = v.contiguous()
        self._values[kind] = v
        return v

    # -- A^T ---------------------------------------------------------------------------
    def _num_cols(self) -> int:
        return self.num_nodes

    def _transposed_graph(self, ptr_t, idx_t, val_t) -> "CSRGraph":
        return CSRGraph(ptr_t, idx_t, val_t)

    def _transpose(self, with_val: bool = False):
        """``(ptr_t, idx_t, order[, val_t])`` of A^T. On the GPU the HIP transposition
        (``ops.csr_transpose``): all int32, ``order`` included, and ``val_t`` the kernel's gather.
        On CPU tensors :func:`_torch_transpose`: ``ptr_t`` and ``order`` int64."""
        if self.ptr.is_cuda:
            return ops.csr_transpose(self.ptr, self.idx, self.val if with_val else None,
                                     self._num_cols())
        ptr_t, rows, order = _torch_transpose(self.ptr, self.idx, self._num_cols(),
                                              self._values.get("edge_rows"))
        idx_t = rows[order].to(torch.int32).contiguous()
        return (ptr_t, idx_t, order) + ((self.val[order],) if with_val else ())

    def transposed(self) -> "CSRGraph":
        """A^T with the same edge values (row = source node), cached: the backward of the
        dense aggregation, dX = A^T dY, runs the same SpMM kernel on it."""
        key = ("transposed", self.val.data_ptr(), ops._version(self.val))
        g = self._values.get(key)
        if g is None:
            st = self._values.get("transposed_structure")
            if st is not None:      # sorted already: the values are gathered
                ptr_t, idx_t, val_t = st[0], st[1], self.val[st[2]]
            elif self.val.requires_grad:    # the gather stays differentiable in val
                ptr_t, idx_t, order = self._transpose()
                val_t = self.val[order.to(torch.int64)]
            else:
                ptr_t, idx_t, _, val_t = self._transpose(with_val=True)
            g = self._transposed_graph(ptr_t, idx_t, val_t)
            self._values = {k: v for k, v in self._values.items()
                            if not (isinstance(k, tuple) and k[0] == "transposed")}
            self._values[key] = g
        return g

    def transposed_structure(self):
        """``(ptr_t, idx_t, order)`` of A^T, cached: edge j of A^T is edge ``order[j]`` of A,
        so changing values are transposed by one gather and no sort."""
        st = self._values.get("transposed_structure")
        if st is None:
            ptr_t, idx_t, order = self._transpose()
            if order.dtype == torch.int32:      # the kernel's: kept as transposed_order()
                self._values.setdefault("transposed_order", order)
            st = (ptr_t.to(torch.int32), idx_t, order.to(torch.int64))
            self._values["transposed_structure"] = st
        return st

    def transposed_order(self) -> torch.Tensor:
        """``transposed_structure()[2]`` as a contiguous int32 ``[E]`` tensor, cached: the
        ``order`` of ``ops.edge_colsum`` (half the bytes of the int64 one per gathered edge)."""
        order = self._values.get("transposed_order")
        if order is None:
            order = self.transposed_structure()[2].to(torch.int32).contiguous()
            order = self._values.setdefault("transposed_order", order)
        return order

    def with_values(self, kind: str) -> "CSRGraph":
        """Same structure with the ``kind`` edge weights (shares ptr/idx, hence the plan)."""
        key = ("graph", kind)
        g = self._values.get(key)
        if g is None:
            g = CSRGraph(self.ptr, self.idx, self.edge_values(kind))
            self._values[key] = g
        return g


def _mask_padding(grad_data, sp_index, count):
    """ref_compat rows fill ``count`` < k slots; the padding slots (0.0f, 0) carry no gradient:
    each is pointed at the row's last filled slot with that slot's gradient, so the scatter
    (last slot wins) never writes into a feature 0 that was not selected."""
    count = count.to(torch.int64)
    k = sp_index.shape[1]
    pad = torch.arange(k, device=count.device)[None, :] >= count[:, None]
    last = (count - 1).clamp(min=0)[:, None]
    g_last = torch.where(count[:, None] > 0, grad_data.gather(1, last),
                         torch.zeros_like(grad_data[:, :1]))
    sp_index = torch.where(pad, sp_index.gather(1, last), sp_index).contiguous()
    grad_data = torch.where(pad, g_last, grad_data).contiguous()
    return grad_data, sp_index


def _fused_forward(plan, x, k, mode, dropout, dense, keep_values):
    """One top-k launch feeding ``plan``'s forward: ``(out, sp_index, count, sp_data)``. Where
    the plan's forward gathers records the top-k writes them (GraphPlan.new_records) next to a
    plain selector table, and the plain ``[N, k]`` value table only with ``keep_values``; else it
    writes the plan's two tables (GraphPlan.new_cbsr). The statistics pair comes with the top-k
    only for a fixed-point forward, the only one that reads it. ``dense``: the ``[N, D]`` tensor
    that receives the dense masked row, or None. ``count`` is None in exact mode, ``sp_data``
    None without ``keep_values``."""
    stats = torch.empty(2, dtype=torch.int32, device=x.device) if plan.fwd_fixed else None
    st2 = stats.view(1, 2) if stats is not None else None
    rec = plan.new_records()
    if rec is not None:
        res = ops.maxk_forward(x, k, mode=mode, return_index=True, records=rec,
                               return_values=keep_values, stats=stats,
                               return_count=mode != "exact", dropout=dropout, dense=dense)
        out = plan.forward_records(rec[0], rec[1], stats=st2)
    else:
        res = ops.maxk_forward(x, k, mode=mode, return_index=True, out=plan.new_cbsr(),
                               stats=stats, return_count=mode != "exact", dropout=dropout,
                               dense=dense)
        out = plan.forward(res[0], res[1], stats=st2)
    return out, res[1], res[2] if len(res) == 3 else None, res[0] if keep_values else None


def _maxk_input_grad(grad_sp, sp_index, count, dim_origin, dropout, g_self):
    """The gradient of the MaxK input from ``grad_sp [N, k]``, the gradient of the kept values
    (None: nothing came through them), and ``g_self [N, D]``, the gradient of the dense masked
    row (or None), merged by one scatter. ``count`` (ref_compat): the filled slots per row. A
    padding slot is pointed at the row's last filled slot with that slot's gradient
    (:func:`_mask_padding`), so the last slot still wins with the same sum; the dropout mask is
    keyed on the feature, so the padding slot gets that slot's mask too."""
    if count is not None:
        if grad_sp is None:
            grad_sp = torch.zeros(sp_index.shape, dtype=torch.float32, device=sp_index.device)
        grad_sp, sp_index = _mask_padding(grad_sp, sp_index, count)
    if g_self is not None:
        g_self = ops._rows_in_place(g_self)
    grad_x = ops.maxk_backward(grad_sp, sp_index, dim_origin=dim_origin, dropout=dropout,
                               grad_dense=g_self)
    if count is not None and g_self is not None:
        # a row that fills no slot (a constant row) has no last filled slot to point at: its
        # slots stay (selector 0, gradient 0), which is harmless without g_self, but the merge
        # would add g_self[r, 0] into a feature 0 that was not selected
        grad_x.masked_fill_((count == 0)[:, None], 0.0)
    return grad_x


class MaxKFunction(torch.autograd.Function):
    """x [N, D] -> CBSR (sp_data, sp_index); backward = the device scatter of grad_data
    into the selected features (the ``grad * mask`` of utils/models.py:23-26).

    ref_compat mode can fill fewer than k slots; the reference pads them with (0.0f, 0)
    (SURVEY §8 a1). Those slots pass no gradient: before the scatter (last slot wins) each
    padding slot is pointed at the row's last filled slot with that slot's gradient, so a
    padding slot never writes (A^T G)[c, 0] into a feature 0 that was not selected."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, k: int, mode: str = "exact", dropout=None):
        x = x.contiguous()
        if mode == "exact":
            sp_data, sp_index = ops.maxk_forward(x, k, mode=mode, return_index=True,
                                                 dropout=dropout)
            ctx.save_for_backward(sp_index)
        else:
            sp_data, sp_index, count = ops.maxk_forward(x, k, mode=mode, return_index=True,
                                                        return_count=True, dropout=dropout)
            ctx.save_for_backward(sp_index, count)
        ctx.dropout = dropout  # (p, seed): the backward recomputes the mask, none is saved
        ctx.dim_origin = x.shape[1]
        ctx.mark_non_differentiable(sp_index)
        return sp_data, sp_index

    @staticmethod
    @first_order_only
    def backward(ctx, grad_data, grad_index):
        saved = ctx.saved_tensors
        grad_x = _maxk_input_grad(grad_data.contiguous(), saved[0],
                                  saved[1] if len(saved) == 2 else None, ctx.dim_origin,
                                  ctx.dropout, None)
        return grad_x, None, None, None


class SpGEMMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sp_data: torch.Tensor, sp_index: torch.Tensor, graph: CSRGraph,
                dim_origin: int):
        k = sp_data.shape[1]
        plan = graph.plan(dim_origin, k)
        out, _ = ops.spgemm_forward(graph.ptr, graph.idx, graph.val, sp_data.contiguous(),
                                    sp_index, graph.num_nodes, graph.num_edges, k,
                                    dim_origin, plan=plan)
        ctx.save_for_backward(sp_index)
        ctx.graph = graph
        ctx.plan = plan  # the backward uses the same plan (no cache lookup, no rebuild)
        ctx.dims = (dim_origin, k)
        _save_values_version(ctx, graph.val)
        return out

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        (sp_index,) = ctx.saved_tensors
        graph = ctx.graph
        dim_origin, k = ctx.dims
        grad_sp = None
        if ctx.needs_input_grad[0]:
            _check_values_version(ctx)
            grad_sp = ops.spgemm_backward(graph.ptr, graph.idx, graph.val,
                                          grad_out.contiguous(), sp_index, graph.num_nodes,
                                          graph.num_edges, k, dim_origin, plan=ctx.plan)
        return grad_sp, None, None, None


class DenseAggFunction(torch.autograd.Function):
    """Y = A X on dense features (DGL ``update_all(copy_u('h'), sum)`` with the graph's edge
    values, i.e. mean / GraphConv normalisation through ``CSRGraph.with_values``): the
    aggregation of the ReLU layers (utils/models.py:140,252 with ``--nonlinear relu``).
    Forward and backward both run ``maxk_dense_spmm_csr``; the backward on A^T."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, graph: CSRGraph):
        ctx.graph = graph
        _save_values_version(ctx, graph.val)
        return ops.dense_spmm(graph.ptr, graph.idx, graph.val, x.contiguous())

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        grad_x = None
        if ctx.needs_input_grad[0]:
            _check_values_version(ctx)
            gt = ctx.graph.transposed()
            grad_x = ops.dense_spmm(gt.ptr, gt.idx, gt.val, grad_out.contiguous())
        return grad_x, None


class MaxKAggregateFunction(torch.autograd.Function):
    """``A @ densify(MaxK(x))`` as one producer-consumer pair (utils/maxk_layers.py:16-34:
    MaxK feeding the SpGEMM), :func:`_fused_forward`. Where the plan's forward gathers records
    (``fwd_layout`` 1, 2 or 4: every default plan that packs), the top-k writes those records
    itself (``maxk_topk_cbsr_records``) next to a plain ``[N, k]`` selector table for the
    backward, and the forward gathers them as they are: it launches no per-call pack or
    statistics pass, and no ``[N, k]`` value table is written. Plans that gather the two plain
    tables (``fwd_layout`` 0 and 3) get plain tables. Backward: the SSpMM on the same plan, then
    :func:`_maxk_input_grad` (same rules as MaxKFunction for ref_compat padding).
    ``dropout=(p, seed)``: feature dropout between the MaxK and the aggregation, inside the
    top-k (records and statistics are those of the dropped values, so still no pack and no
    statistics pass) and inside the scatter; the pair is kept on ``ctx``, no mask tensor."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, graph: CSRGraph, k: int, mode: str = "exact",
                dropout=None):
        x = x.contiguous()
        plan = graph.plan(x.shape[1], k)
        out, sp_index, count, _ = _fused_forward(plan, x, k, mode, dropout, None, False)
        ctx.save_for_backward(sp_index, *(() if count is None else (count,)))
        ctx.plan = plan
        ctx.dropout = dropout
        ctx.dim_origin = x.shape[1]
        _save_values_version(ctx, graph.val)
        return out

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        grad_x = None
        if ctx.needs_input_grad[0]:
            _check_values_version(ctx)
            grad_sp = ctx.plan.backward(grad_out.contiguous(), saved[0])
            grad_x = _maxk_input_grad(grad_sp, saved[0], saved[1] if len(saved) == 2 else None,
                                      ctx.dim_origin, ctx.dropout, None)
        return grad_x, None, None, None, None


class MaxKSelfAggregateFunction(torch.autograd.Function):
    """``(x_m, A @ x_m)`` with ``x_m = dropout(x * topk_mask(x))`` dense ``[N, D]``: the pair a
    layer with a self term needs (``fc_self(x_m)`` in GraphSAGE, ``(1 + eps) x_m`` in GIN) from
    one top-k launch. Forward as :class:`MaxKAggregateFunction` (records, or plain tables for
    plans that gather those; the statistics pair only for a fixed-point forward), with the
    top-k also storing the dense masked row from the registers that hold it
    (``maxk_topk_cbsr_dense``): no ``densify`` fill and scatter, no pack, no statistics pass.
    Only the selectors are saved (and the slot counts in ref_compat mode). Backward: the SSpMM
    when the aggregated output has a gradient, then one scatter that adds the dense output's
    gradient at the selected features before the dropout factor
    (``maxk_scatter_backward_merge``): no gather of ``densify``'s gradient, no ``[N, k]`` add."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, graph: CSRGraph, k: int, mode: str = "exact",
                dropout=None):
        x = x.contiguous()
        plan = graph.plan(x.shape[1], k)
        x_m = torch.empty_like(x)
        out, sp_index, count, _ = _fused_forward(plan, x, k, mode, dropout, x_m, False)
        ctx.save_for_backward(sp_index, *(() if count is None else (count,)))
        ctx.plan = plan
        ctx.dropout = dropout
        ctx.dim_origin = x.shape[1]
        _save_values_version(ctx, graph.val)
        ctx.set_materialize_grads(False)  # an unused output arrives as None, not as zeros
        return x_m, out

    @staticmethod
    @first_order_only
    def backward(ctx, g_self, g_agg):
        saved = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_self is None and g_agg is None):
            return None, None, None, None, None
        grad_sp = None
        if g_agg is not None:
            _check_values_version(ctx)
            grad_sp = ctx.plan.backward(g_agg.contiguous(), saved[0])
        grad_x = _maxk_input_grad(grad_sp, saved[0], saved[1] if len(saved) == 2 else None,
                                  ctx.dim_origin, ctx.dropout, g_self)
        return grad_x, None, None, None, None


class EdgeWeightedFunction(torch.autograd.Function):
    """The aggregation with the edge values as an explicit differentiable input ``val [E]`` (the
    effective values ``graph.val * edge_weight``), for the three entry points that take
    ``edge_weight=``. ``form``:

    * ``"spgemm"``: ``feat`` is ``sp_data`` (with ``sp_index`` and ``dim_origin``) -> ``out``;
    * ``"aggregate"``: ``feat`` is dense ``x`` -> ``out``, as :class:`MaxKAggregateFunction`;
    * ``"self"``: ``feat`` is dense ``x`` -> ``(x_m, out)``, as :class:`MaxKSelfAggregateFunction`.

    Forward: the kernels of those Functions on ``graph.weighted_plan``, value-refreshed to
    ``val``. The plain ``[N, k]`` value table of the fused forms is emitted and saved only when
    ``val`` needs a gradient. Backward: the SSpMM and the scatter as there, plus
    ``ops.spgemm_edge_grad`` for ``val`` when asked. The plan's value snapshot is shared by
    every weighted call on the graph, so the backward re-refreshes it when another call's values
    are in it; ``val`` is kept on ``ctx`` for that."""

    @staticmethod
    def forward(ctx, feat, val, graph, form, sp_index, dim_origin, k, mode, dropout):
        feat, val = feat.contiguous(), val.contiguous()
        need_val = ctx.needs_input_grad[1]
        d = dim_origin if form == "spgemm" else feat.shape[1]
        k = feat.shape[1] if form == "spgemm" else k
        plan = graph.weighted_plan(d, k)
        plan.refresh_values(val)
        x_m = count = None
        if form == "spgemm":
            sp_data = feat
            out, _ = ops.spgemm_forward(graph.ptr, graph.idx, val, sp_data, sp_index,
                                        graph.num_nodes, graph.num_edges, k, d, plan=plan)
        else:
            x_m = torch.empty_like(feat) if form == "self" else None
            out, sp_index, count, sp_data = _fused_forward(plan, feat, k, mode, dropout, x_m,
                                                           need_val)
        ctx.save_for_backward(sp_index, *(() if count is None else (count,)),
                              *((sp_data,) if need_val else ()))
        ctx.has_count, ctx.has_data = count is not None, need_val
        ctx.graph, ctx.plan, ctx.val = graph, plan, val
        ctx.form, ctx.dropout, ctx.dims = form, dropout, (d, k)
        ctx.set_materialize_grads(False)  # an unused output arrives as None, not as zeros
        return (x_m, out) if form == "self" else out

    @staticmethod
    @first_order_only
    def backward(ctx, *grads):
        none = (None,) * 7
        g_agg = grads[-1]
        g_self = grads[0] if ctx.form == "self" else None
        saved = ctx.saved_tensors
        sp_index = saved[0]
        count = saved[1] if ctx.has_count else None
        graph, plan, val = ctx.graph, ctx.plan, ctx.val
        d, k = ctx.dims
        grad_val = grad_feat = None
        if g_agg is not None:
            g_agg = g_agg.contiguous()
            if ctx.needs_input_grad[1]:
                grad_val = ops.spgemm_edge_grad(graph.ptr, graph.idx, g_agg, saved[-1], sp_index,
                                                graph.num_nodes, graph.num_edges, k, d)
        if ctx.needs_input_grad[0] and (g_agg is not None or g_self is not None):
            grad_sp = None
            if g_agg is not None:
                if ops._values_stale(plan, val):
                    plan.refresh_values(val)  # another weighted call ran on this graph since
                grad_sp = plan.backward(g_agg, sp_index)
            if ctx.form == "spgemm":
                return (grad_sp, grad_val) + none
            grad_feat = _maxk_input_grad(grad_sp, sp_index, count, d, ctx.dropout, g_self)
        return (grad_feat, grad_val) + none


class DenseEdgeWeightedFunction(torch.autograd.Function):
    """:class:`DenseAggFunction` with the edge values as a differentiable input ``val [E]``:
    ``Y = A(val) X`` (the ReLU layers with ``edge_weight=``). Backward: ``dX = A(val)^T dY`` by
    the same SpMM on the cached transposed structure (the values are gathered, not re-sorted),
    and ``d val`` by ``ops.spgemm_edge_grad`` run with ``k = D`` on ``X`` itself as the value
    table and identity selectors (so D % 4 == 0 and D <= 256 when ``val`` needs a gradient)."""

    @staticmethod
    def forward(ctx, x, val, graph):
        x, val = x.contiguous(), val.contiguous()
        ctx.graph = graph
        ctx.save_for_backward(val, *((x,) if ctx.needs_input_grad[1] else ()))
        return ops.dense_spmm(graph.ptr, graph.idx, val, x)

    @staticmethod
    @first_order_only
    def backward(ctx, grad_out):
        saved, graph = ctx.saved_tensors, ctx.graph   # read once (checkpoint unpacks per read)
        val = saved[0]
        grad_out = grad_out.contiguous()
        grad_x = grad_val = None
        if ctx.needs_input_grad[0]:
            ptr_t, idx_t, order = graph.transposed_structure()
            grad_x = ops.dense_spmm(ptr_t, idx_t, val[order], grad_out)
        if ctx.needs_input_grad[1]:
            x = saved[1]
            n, d = x.shape
            ident = torch.arange(d, dtype=torch.uint8, device=x.device).repeat(n, 1)
            grad_val = ops.spgemm_edge_grad(graph.ptr, graph.idx, grad_out, x, ident, n,
                                            graph.num_edges, d, d)
        return grad_x, grad_val, None


class EdgeSoftmaxFunction(torch.autograd.Function):
    """Softmax of per-edge logits over each destination row's in-edges (DGL's
    ``edge_softmax``): ``ops.edge_softmax`` forward, ``ops.edge_softmax_backward`` backward. Only
    the output is saved: the gradient ``y * (g - sum_row(y g))`` needs no logits."""

    @staticmethod
    def forward(ctx, graph: CSRGraph, logits: torch.Tensor):
        y = ops.edge_softmax(graph.ptr, logits.contiguous())
        ctx.save_for_backward(y)
        ctx.graph = graph
        ctx.set_materialize_grads(False)  # an unused output arrives as None, not as zeros
        return y

    @staticmethod
    @first_order_only
    def backward(ctx, grad_y):
        if grad_y is None or not ctx.needs_input_grad[1]:
            return None, None
        (y,) = ctx.saved_tensors
        return None, ops.edge_softmax_backward(ctx.graph.ptr, y, grad_y.contiguous())


def edge_softmax(graph: CSRGraph, logits: torch.Tensor) -> torch.Tensor:
    """``alpha[e] = exp(logits[e]) / sum_{e' into row(e)} exp(logits[e'])`` for f32 ``[E]``
    logits in the CSRGraph's own edge order, differentiable in ``logits`` (DGL's
    ``edge_softmax`` over the in-edges; EdgeSoftmaxFunction). The result is an ``edge_weight=``
    of the aggregations: attention."""
    if not (isinstance(logits, torch.Tensor) and logits.dtype == torch.float32 and
            logits.shape == (graph.num_edges,) and logits.device == graph.device):
        raise RuntimeError("logits must be a float32 [num_edges] tensor on the graph's device, "
                           "in the CSRGraph's edge order")
    return EdgeSoftmaxFunction.apply(graph, logits)


def _effective_values(graph: CSRGraph, edge_weight: torch.Tensor) -> torch.Tensor:
    """``graph.val * edge_weight`` (a torch multiply: the chain rule to ``edge_weight`` is
    torch's); ``edge_weight`` is f32 ``[E]`` on the graph's device, in the CSRGraph's edge order."""
    if not (isinstance(edge_weight, torch.Tensor) and edge_weight.dtype == torch.float32 and
            edge_weight.shape == (graph.num_edges,) and edge_weight.device == graph.device):
        raise RuntimeError("edge_weight must be a float32 [num_edges] tensor on the graph's "
                           "device, in the CSRGraph's edge order")
    return graph.val * edge_weight


def dense_aggregate(x: torch.Tensor, graph: CSRGraph,
                    edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y = A @ x for dense x (ReLU layers), differentiable in x, and in ``edge_weight`` (the
    edge values are then ``graph.val * edge_weight``) when one is given."""
    if edge_weight is not None:
        return DenseEdgeWeightedFunction.apply(x, _effective_values(graph, edge_weight), graph)
    return DenseAggFunction.apply(x, graph)


def densify(sp_data: torch.Tensor, sp_index: torch.Tensor, dim_origin: int) -> torch.Tensor:
    """Dense ``[N, D]`` view of CBSR features (differentiable in sp_data; duplicate
    selectors sum, as in the kernels)."""
    out = torch.zeros((sp_data.shape[0], dim_origin), dtype=sp_data.dtype,
                      device=sp_data.device)
    return out.scatter_add(1, sp_index.long(), sp_data)


def _dropout_pair(dropout_p: float, training: bool, seed):
    """The ``(p, seed)`` pair of a fused-dropout call, or ``None`` when nothing is dropped.
    ``seed=None`` draws one int64 from torch's CPU default generator: reproducible under
    ``torch.manual_seed``, and no device sync. The seed is a launch argument, so a step captured
    into a graph replays the mask of capture time: an explicit ``seed`` means exactly that and
    is accepted; drawing one during capture is refused (``F.dropout``, which the fused dropout
    replaces, draws a fresh mask on every replay)."""
    if not training or dropout_p == 0:
        return None
    if not 0.0 <= dropout_p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout_p}")
    if seed is None:
        ops._refuse_capture("fused dropout with seed=None (a seed drawn on the host)",
                            "pass seed=; a captured step replays one mask")
        seed = torch.empty((), dtype=torch.int64).random_().item()
    return float(dropout_p), int(seed)


def maxk(x: torch.Tensor, k: int, mode: str = "exact", dropout_p: float = 0.0,
         training: bool = True, seed: Optional[int] = None):
    """(sp_data, sp_index) = MaxK(x), differentiable in x. With ``dropout_p > 0`` and
    ``training``, feature dropout on the kept values inside the top-k kernel (and its scatter in
    the backward): ``sp_data`` holds ``keep ? x / (1 - p) : 0`` with the counter-based mask of
    include/maxk_hip.h for ``seed`` (``None``: drawn from torch's CPU generator)."""
    return MaxKFunction.apply(x, k, mode, _dropout_pair(dropout_p, training, seed))


def spgemm(sp_data: torch.Tensor, sp_index: torch.Tensor, graph: CSRGraph,
           dim_origin: int, edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y = A @ densify(sp_data, sp_index), differentiable in sp_data. ``edge_weight``: f32
    ``[E]`` on the graph's device, in the CSRGraph's own edge order; the edge values are then
    ``graph.val * edge_weight`` and Y is differentiable in ``edge_weight`` too (DGL's
    ``u_mul_e``; EdgeWeightedFunction). ``None`` is the path without it, unchanged."""
    if edge_weight is not None:
        return EdgeWeightedFunction.apply(sp_data, _effective_values(graph, edge_weight), graph,
                                          "spgemm", sp_index, dim_origin, None, None, None)
    return SpGEMMFunction.apply(sp_data, sp_index, graph, dim_origin)


def maxk_aggregate(x: torch.Tensor, graph: CSRGraph, k: int, mode: str = "exact",
                   dropout_p: float = 0.0, training: bool = True,
                   seed: Optional[int] = None,
                   edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused MaxK + aggregation: ``A @ (x * topk_mask(x))`` (DGL: MaxK.apply then
    update_all(u_mul_e, sum) with edge weights ``graph.val``), differentiable in x; the
    top-k writes the records the forward gathers, and the statistics a fixed-point forward
    needs (MaxKAggregateFunction). ``dropout_p``, ``training``, ``seed`` as for :func:`maxk`:
    ``A @ dropout(x * topk_mask(x))`` with the dropout inside the top-k and the scatter, and
    still no pack or statistics pass. ``edge_weight`` as for :func:`spgemm`."""
    if edge_weight is not None:
        return EdgeWeightedFunction.apply(x, _effective_values(graph, edge_weight), graph,
                                          "aggregate", None, None, k, mode,
                                          _dropout_pair(dropout_p, training, seed))
    return MaxKAggregateFunction.apply(x, graph, k, mode,
                                       _dropout_pair(dropout_p, training, seed))


def maxk_self_aggregate(x: torch.Tensor, graph: CSRGraph, k: int, mode: str = "exact",
                        dropout_p: float = 0.0, training: bool = True,
                        seed: Optional[int] = None,
                        edge_weight: Optional[torch.Tensor] = None):
    """``(x_masked [N, D], agg [N, D])``: ``x_masked = dropout(x * topk_mask(x))`` dense and
    ``agg = A @ x_masked``, both differentiable in x (MaxKSelfAggregateFunction): what
    ``maxk`` → ``densify`` → ``spgemm`` computes, from one top-k launch that writes the dense
    row, the forward's records and their statistics, and with one scatter in the backward that
    merges both outputs' gradients. ``agg`` is :func:`maxk_aggregate` of the same arguments,
    bit for bit. ``dropout_p``, ``training``, ``seed`` as for :func:`maxk`; ``edge_weight`` as
    for :func:`spgemm` (it weights ``agg`` only)."""
    if edge_weight is not None:
        return EdgeWeightedFunction.apply(x, _effective_values(graph, edge_weight), graph, "self",
                                          None, None, k, mode,
                                          _dropout_pair(dropout_p, training, seed))
    return MaxKSelfAggregateFunction.apply(x, graph, k, mode,
                                           _dropout_pair(dropout_p, training, seed))
