"""Drop-in MaxK graph layers on the gfx950 SpGEMM / SSpMM kernels.

Replaces the reference's ``MaxKSAGEConv`` (utils/maxk_layers.py:47-265) and
``MaxKGCNConv`` (utils/maxk_layers.py:267-448) with the same constructor signatures, and
``MaxKSAGE`` / ``MaxKGCN`` / ``MaxKGIN`` (utils/integrated_models.py:8-271, imported by
maxk_gnn_integrated.py:21 and built with the kwargs of :317-332) with the same
constructors, but with the SURVEY §8(b) caller defects fixed:

* MaxK yields CBSR ``(sp_data, sp_index)`` directly; no dense ``[N, k]`` misuse, no
  per-row Python ``_extract_sparse_format`` loop, no uint8 wrap (D <= 256 is checked);
* the aggregation runs over the in-edge CSR (destination rows) and is differentiable:
  SpGEMM forward, SSpMM backward, MaxK backward scatter;
* edge weights are built on the device once per graph (no per-row ``.item()`` loop).

Numerics follow DGL on the same inputs (the semantics the reference trained with,
utils/models.py:109-411 + dglnn.SAGEConv / GraphConv / GINConv):

* ``nonlinear="maxk"`` (default): MaxK feeds the SpGEMM kernels.
  - ``MaxKSAGEConv``: ``rst = fc_self(x) + fc_neigh(mean_{u->v} x_u) (+ bias)``, then
    ``norm``; ``x = feat_drop(MaxK(feat))``. Dropout acts on the k kept values only (the
    other entries are zero either way). The reference's layer applies MaxK after
    ``fc_neigh`` and dropout to its output (maxk_layers.py:85-88,183);
    ``maxk_after_fc=True`` keeps that ordering. ``aggregator_type="pool"``:
    ``rst = fc_self(x) + fc_neigh(max_{u->v} MaxK(fc_pool(x_u)))``, MaxK in the place of
    DGL's ReLU after ``fc_pool`` and the max taken by the max-aggregation kernels
    (:mod:`maxk_kernels.pooling`; ``nonlinear="relu"``: ``max ReLU(fc_pool(x_u))`` on dense
    rows, the same kernels with ``k = D``); it takes no ``edge_weight``.
    ``aggregator_type="gcn"``: ``rst = fc_neigh((sum_{u->v} x_u + x_v) / (in_deg_v + 1))``
    without ``fc_self``, as in DGL.
  - ``MaxKGCNConv``: ``rst = A_norm MaxK(feat W) (+ bias)`` with ``A_norm`` the GraphConv
    normalisation ('both', 'right', 'left', 'none'); with ``weight=False`` this is
    ``dglnn.GraphConv(weight=None)`` applied to ``MaxK(feat)``.
  - ``MaxKGINConv``: ``rst = (1 + eps) x + sum_{u->v} x_u`` on ``x = MaxK(feat)``
    (``dglnn.GINConv(learn_eps=True, activation=None)``, utils/models.py:373).
* ``nonlinear="relu"`` (``--nonlinear relu``, utils/config.py:47): the models apply ReLU
  themselves and the layers aggregate the dense features with the HIP CSR SpMM
  (``maxk_dense_spmm_csr``; backward on the transposed CSR), i.e. the plain DGL layers
  of utils/models.py (``dglnn.SAGEConv(mean)``, ``GraphConv(weight=None)``, ``GINConv``).

``fused_dropout=True`` (every layer and model; default off) moves the ``feat_drop`` of the
``nonlinear="maxk"`` path into the kernels: in training mode with ``feat_drop > 0`` the
top-k emits the dropped, scaled values and the MaxK scatter applies the same mask in the
backward (a counter-based mask of (seed, row, feature), include/maxk_hip.h; one seed per
layer call from torch's CPU generator), so no ``F.dropout`` pass runs, no mask is saved, and
GCN and the SAGE ``maxk_after_fc`` branch stay on the fused ``maxk_aggregate`` pair. It is
the same distribution but other random numbers than ``F.dropout`` draws, which is why it is
opt-in here; a later change may make it the default. Eval mode and ``feat_drop == 0`` do not
depend on it.

Layers with a self term (``MaxKSAGEConv`` in its default ordering, ``MaxKGINConv``) need
``x = feat_drop(MaxK(feat))`` twice, aggregated and dense. Whenever no ``F.dropout`` has to sit
between MaxK and the aggregation (``feat_drop == 0``, eval mode, or ``fused_dropout=True``)
they take both from ``maxk_self_aggregate``: the top-k writes the dense masked row next to the
forward's records, and one scatter merges both gradients in the backward (no ``densify``, no
per-call pack or statistics pass, no ``[N, k]`` value table saved). Training with
``feat_drop > 0`` and ``fused_dropout=False`` keeps the composition ``maxk`` → ``F.dropout`` →
``densify`` / ``spgemm``, because it draws ``F.dropout``'s random numbers.

``norm`` of ``MaxKSAGEConv`` may be a module instance (DGL's convention) or a class that is
instantiated as ``norm(out_feats)`` (utils/maxk_layers.py:66-67).

``graph`` may be a :class:`~maxk_kernels.autograd.CSRGraph` or a DGL graph (converted
with ``adj_tensors('csc')`` when DGL is installed; it is not required).

``edge_weight`` (every layer's and model's ``forward``; DGL's argument of the same name): an
f32 ``[E]`` tensor in the CSRGraph's own edge order. As in DGL the degree normalisation comes
from the unweighted degrees and each edge's message is multiplied by its weight (``u_mul_e``),
and the output is differentiable in it, on both nonlinear paths: the SDDMM kernel
(``maxk_sddmm_edge_grad``) gives its gradient, for ``nonlinear="relu"`` run with ``k = D`` on
the dense features with identity selectors. It needs a CSRGraph: with a DGL graph it raises
``TypeError``, because the edge-id permutation between the two orders is not mapped.

Sampled blocks (:mod:`maxk_kernels.sampling`): ``MaxKSAGEConv.forward(block, feat)`` takes
``feat [num_src, in]`` to ``[num_dst, out]`` for the ``mean`` and ``sum`` aggregators on both
``nonlinear`` paths, with the neighbour term over the block's sampled edges and the self term from
the first ``num_dst`` rows of the masked input; ``MaxKSAGE.forward(blocks, x)`` takes one block
per layer, outermost first. Every other aggregator, layer and model, and ``edge_weight=``, raise
``NotImplementedError`` for a block.

``MaxKGATConv`` is the layer that ``edge_weight=`` and the edge softmax (``edge_softmax``,
``maxk_edge_softmax_forward`` / ``_backward``) make possible: single-head graph attention
(``dglnn.GATConv`` with one head) whose messages are the MaxK features.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .autograd import (CSRGraph, dense_aggregate, densify, edge_softmax, maxk, maxk_aggregate,
                       maxk_self_aggregate, spgemm)
from .attention import gat_attention
from .heads import gat_attention_heads, heads_aggregate, maxk_heads_aggregate
from .pooling import dense_max_aggregate, maxk_max_aggregate
from .sampling import Block, block_aggregate, block_self_aggregate, block_spgemm

NONLINEAR = ("maxk", "relu")


def as_csr(graph, edge_weight=None) -> CSRGraph:
    if isinstance(graph, CSRGraph):
        return graph
    if edge_weight is not None:
        raise TypeError("edge_weight needs a maxk_kernels.CSRGraph: the weights follow the "
                        "CSRGraph's own edge order, and a DGL graph's edge ids are not mapped to it")
    if hasattr(graph, "adj_tensors"):
        return CSRGraph.from_dgl(graph)
    raise TypeError("graph must be a maxk_kernels.CSRGraph or a DGL graph")


BLOCK_SUPPORT = ("sampled blocks are supported by MaxKSAGEConv and MaxKSAGE with "
                 'aggregator_type "mean" or "sum", without edge_weight')


def _refuse_block(graph, who: str) -> None:
    """Layers without a block path refuse a Block (or a list of them) by name."""
    if isinstance(graph, Block) or (isinstance(graph, (list, tuple)) and graph and
                                    all(isinstance(b, Block) for b in graph)):
        raise NotImplementedError(f"{who} does not take a Block: {BLOCK_SUPPORT}")


def _check_nonlinear(nonlinear: str) -> str:
    if nonlinear not in NONLINEAR:
        raise ValueError(f"nonlinear must be one of {NONLINEAR} (utils/config.py:47), "
                         f"got {nonlinear!r}")
    return nonlinear


def _sparse_dropout(sp_data: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    return F.dropout(sp_data, p, training) if p > 0 else sp_data


def _maxk_dropout(layer, feat: torch.Tensor):
    """``feat_drop(MaxK(feat))`` as CBSR for a layer: the dropout inside the top-k kernel with
    ``fused_dropout``, else ``F.dropout`` on the ``[N, k]`` values."""
    if layer.fused_dropout:
        return maxk(feat, layer.maxk, layer.topk_mode, dropout_p=layer.feat_drop,
                    training=layer.training)
    sp_data, sp_index = maxk(feat, layer.maxk, layer.topk_mode)
    return _sparse_dropout(sp_data, layer.feat_drop, layer.training), sp_index


def _maxk_self_pair(layer, feat: torch.Tensor, csr: CSRGraph, edge_weight=None):
    """``(x, A @ x)`` with ``x = feat_drop(MaxK(feat))`` dense, for a layer with a self term:
    ``maxk_self_aggregate`` unless ``F.dropout`` has to sit between MaxK and the aggregation
    (training with ``feat_drop > 0`` and no ``fused_dropout``)."""
    if layer.feat_drop > 0 and layer.training and not layer.fused_dropout:
        sp_data, sp_index = _maxk_dropout(layer, feat)
        return (densify(sp_data, sp_index, layer.in_feats),
                spgemm(sp_data, sp_index, csr, layer.in_feats, edge_weight=edge_weight))
    return maxk_self_aggregate(feat, csr, layer.maxk, layer.topk_mode,
                               dropout_p=layer.feat_drop, training=layer.training,
                               edge_weight=edge_weight)


def _make_norm(norm, out_feats):
    """DGL passes a module instance; the reference layer passes a class and calls
    ``norm(out_feats)`` (utils/maxk_layers.py:66-67). Accept both."""
    if norm is None:
        return None
    if isinstance(norm, type):
        return norm(out_feats)
    return norm


class MaxKSAGEConv(nn.Module):
    """GraphSAGE layer with MaxK sparsity and the fused aggregation kernels.

    Signature of utils/maxk_layers.py:51-52 plus ``bias`` (dglnn.SAGEConv has one),
    ``maxk_after_fc`` (the reference layer's MaxK placement) and ``nonlinear``.
    """

    def __init__(self, in_feats, out_feats, aggregator_type="mean", feat_drop=0., norm=None,
                 maxk=32, bias=True, maxk_after_fc=False, topk_mode="exact",
                 nonlinear="maxk", fused_dropout=False):
        super().__init__()
        self.fused_dropout = bool(fused_dropout)
        if aggregator_type not in ("mean", "sum", "pool", "gcn"):
            raise ValueError(f"Unsupported aggregator type: {aggregator_type}")
        if maxk_after_fc and aggregator_type in ("pool", "gcn"):
            raise ValueError(f"maxk_after_fc is not defined for the {aggregator_type} aggregator")
        self.in_feats = in_feats
        self.out_feats = out_feats
        self.aggregator_type = aggregator_type
        self.maxk = maxk
        self.maxk_after_fc = maxk_after_fc
        self.topk_mode = topk_mode
        self.nonlinear = _check_nonlinear(nonlinear)
        if aggregator_type != "gcn":  # DGL's gcn aggregator has no self weight
            self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_feats)) if bias else None
        self.norm = _make_norm(norm, out_feats)
        self.feat_drop = float(feat_drop)
        if aggregator_type == "pool":  # after the existing parameters: their stream is unchanged
            self.fc_pool = nn.Linear(in_feats, in_feats)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if self.aggregator_type != "gcn":
            nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)
        if self.bias is not None:
            nn.init.zeros_(self.bias)
        if self.aggregator_type == "pool":
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)

    def _forward_pool(self, graph, feat: torch.Tensor, edge_weight) -> torch.Tensor:
        """dglnn.SAGEConv("pool"): ``fc_self(x) + fc_neigh(max_{u->v} act(fc_pool(x_u)))`` with
        MaxK in the place of DGL's ReLU on the ``nonlinear="maxk"`` path."""
        if edge_weight is not None:
            raise NotImplementedError("the pool aggregator takes no edge_weight (a weighted max "
                                      "is not defined here)")
        csr = as_csr(graph)
        if self.nonlinear == "relu":
            x = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
            neigh = dense_max_aggregate(F.relu(self.fc_pool(x)), csr)
        else:
            sp_data, sp_index = _maxk_dropout(self, feat)
            x = densify(sp_data, sp_index, self.in_feats)
            neigh = maxk_max_aggregate(self.fc_pool(x), csr, self.maxk, self.topk_mode)
        return self.fc_self(x) + self.fc_neigh(neigh)

    def _forward_gcn(self, graph, feat: torch.Tensor, ew) -> torch.Tensor:
        """dglnn.SAGEConv("gcn"): ``fc_neigh((sum_{u->v} x_u + x_v) / (in_deg_v + 1))``;
        ``edge_weight`` multiplies the messages only."""
        csr = as_csr(graph, ew).with_values("sum")
        if self.nonlinear == "relu":
            x = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
            neigh = dense_aggregate(x, csr, ew)
        else:
            x, neigh = _maxk_self_pair(self, feat, csr, ew)
        deg = (csr.in_degrees() + 1).to(feat.dtype).unsqueeze(1)
        return self.fc_neigh((neigh + x) / deg)

    def _forward_block(self, block: Block, feat: torch.Tensor, edge_weight) -> torch.Tensor:
        """``feat [num_src, in] -> [num_dst, out]`` on a sampled block: the neighbour term over
        the sampled edges (``block_aggregate``: MaxK, then the plan-less weighted sum), the self
        term from the first ``num_dst`` rows of the masked input."""
        if self.aggregator_type not in ("mean", "sum"):
            raise NotImplementedError(f'MaxKSAGEConv with aggregator_type "{self.aggregator_type}"'
                                      f" does not take a Block: {BLOCK_SUPPORT}")
        if edge_weight is not None:
            raise NotImplementedError("MaxKSAGEConv with edge_weight does not take a Block: "
                                      f"{BLOCK_SUPPORT}")
        blk = block.with_values(self.aggregator_type)
        nd = blk.num_dst
        drop = self.feat_drop > 0 and self.training
        if self.nonlinear == "relu":
            # dense rows through the same kernels with k = D (identity selection)
            x = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
            rst = self.fc_self(x[:nd]) + self.fc_neigh(block_aggregate(x, blk, x.shape[1]))
        elif self.maxk_after_fc:
            h_self = self.fc_self(feat[:nd])
            if drop and not self.fused_dropout:
                sp_data, sp_index = maxk(self.fc_neigh(feat), self.maxk, self.topk_mode)
                sp_data = _sparse_dropout(sp_data, self.feat_drop, self.training)
                rst = h_self + block_spgemm(sp_data, sp_index, blk, self.out_feats)
            else:
                rst = h_self + block_aggregate(self.fc_neigh(feat), blk, self.maxk,
                                               self.topk_mode, dropout_p=self.feat_drop,
                                               training=self.training)
        else:
            if drop and not self.fused_dropout:
                sp_data, sp_index = _maxk_dropout(self, feat)
                x = densify(sp_data, sp_index, self.in_feats)
                neigh = block_spgemm(sp_data, sp_index, blk, self.in_feats)
            else:
                x, neigh = block_self_aggregate(feat, blk, self.maxk, self.topk_mode,
                                                dropout_p=self.feat_drop, training=self.training)
            rst = self.fc_self(x[:nd]) + self.fc_neigh(neigh)
        if self.bias is not None:
            rst = rst + self.bias
        return self.norm(rst) if self.norm is not None else rst

    def forward(self, graph, feat: torch.Tensor, edge_weight=None) -> torch.Tensor:
        ew = edge_weight
        if isinstance(graph, Block):
            return self._forward_block(graph, feat, ew)
        if self.aggregator_type in ("pool", "gcn"):
            rst = (self._forward_pool if self.aggregator_type == "pool"
                   else self._forward_gcn)(graph, feat, ew)
            if self.bias is not None:
                rst = rst + self.bias
            return self.norm(rst) if self.norm is not None else rst
        csr = as_csr(graph, ew).with_values(self.aggregator_type)
        if self.nonlinear == "relu":
            # dglnn.SAGEConv(mean) on dense features (the model applied the ReLU)
            x = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
            rst = self.fc_self(x) + self.fc_neigh(dense_aggregate(x, csr, ew))
        elif self.maxk_after_fc:
            # reference ordering (maxk_layers.py:85-88): MaxK(fc_neigh(feat)) aggregated
            h_self = self.fc_self(feat)
            if self.feat_drop > 0 and self.training and self.fused_dropout:
                rst = h_self + maxk_aggregate(self.fc_neigh(feat), csr, self.maxk, self.topk_mode,
                                              dropout_p=self.feat_drop, edge_weight=ew)
            elif self.feat_drop > 0 and self.training:
                sp_data, sp_index = maxk(self.fc_neigh(feat), self.maxk, self.topk_mode)
                sp_data = _sparse_dropout(sp_data, self.feat_drop, self.training)
                rst = h_self + spgemm(sp_data, sp_index, csr, self.out_feats, edge_weight=ew)
            else:  # no dropout between MaxK and the SpGEMM: the fused producer-consumer pair
                rst = h_self + maxk_aggregate(self.fc_neigh(feat), csr, self.maxk, self.topk_mode,
                                              edge_weight=ew)
        else:
            x, neigh = _maxk_self_pair(self, feat, csr, ew)
            rst = self.fc_self(x) + self.fc_neigh(neigh)
        if self.bias is not None:
            rst = rst + self.bias
        if self.norm is not None:
            rst = self.norm(rst)
        return rst


class MaxKGCNConv(nn.Module):
    """GCN layer with MaxK sparsity (signature of utils/maxk_layers.py:271-272, plus
    ``feat_drop``: dropout between MaxK and the aggregation, as utils/models.py:262-264,
    and ``nonlinear``)."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True,
                 allow_zero_in_degree=False, maxk=32, topk_mode="exact", feat_drop=0.,
                 nonlinear="maxk", fused_dropout=False):
        super().__init__()
        self.fused_dropout = bool(fused_dropout)
        if norm not in ("both", "right", "left", "none"):
            raise ValueError(f"Invalid norm value {norm!r}")
        self.in_feats = in_feats
        self.out_feats = out_feats
        self.norm = norm
        self.maxk = maxk
        self.topk_mode = topk_mode
        self.nonlinear = _check_nonlinear(nonlinear)
        self.allow_zero_in_degree = allow_zero_in_degree
        self.feat_drop = float(feat_drop)
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats)) if weight else None
        self.bias = nn.Parameter(torch.empty(out_feats)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight is not None:
            nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, graph, feat: torch.Tensor, edge_weight=None) -> torch.Tensor:
        _refuse_block(graph, "MaxKGCNConv")
        ew = edge_weight
        csr = as_csr(graph, ew)
        if not self.allow_zero_in_degree and bool((csr.in_degrees() == 0).any()):
            raise ValueError("Graph has nodes with zero in-degree")
        if self.weight is not None:
            feat = feat @ self.weight
        if self.nonlinear == "relu":
            x = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
            rst = dense_aggregate(x, csr.with_values(self.norm), ew)
        elif self.feat_drop > 0 and self.training and self.fused_dropout:
            rst = maxk_aggregate(feat, csr.with_values(self.norm), self.maxk, self.topk_mode,
                                 dropout_p=self.feat_drop, edge_weight=ew)
        elif self.feat_drop > 0 and self.training:
            sp_data, sp_index = maxk(feat, self.maxk, self.topk_mode)
            sp_data = _sparse_dropout(sp_data, self.feat_drop, self.training)
            rst = spgemm(sp_data, sp_index, csr.with_values(self.norm), feat.shape[1],
                         edge_weight=ew)
        else:
            rst = maxk_aggregate(feat, csr.with_values(self.norm), self.maxk, self.topk_mode,
                                 edge_weight=ew)
        if self.bias is not None:
            rst = rst + self.bias
        return rst


class MaxKGATConv(nn.Module):
    """Single-head graph attention (``dglnn.GATConv(num_heads=1)`` without residual or
    activation) on MaxK features, ``[N, in_feats] -> [N, out_feats]``:

        h = fc(feat);  el = <h, attn_l>;  er = <h, attn_r>        (the dense h, before MaxK)
        e_uv = leaky_relu(el_u + er_v);  alpha = attn_drop(edge_softmax(e))
        rst_v = sum_{u->v} alpha_uv * feat_drop(MaxK(h))_u + bias

    The softmax over each node's in-edges is the HIP pair behind :func:`edge_softmax`, the
    aggregation ``maxk_aggregate(..., edge_weight=alpha)`` on the unit-valued graph with the
    ``feat_drop`` / ``fused_dropout`` branches of :class:`MaxKGCNConv`; ``nonlinear="relu"``
    aggregates the dense ``h`` (``dense_aggregate``). The score gather ``el[idx] +
    er[edge_rows]`` and its gradient are torch's; with ``fused_attention=True`` (default off)
    the gather, add, leaky-relu and softmax are the one kernel of :func:`gat_attention` and the
    score gradients its two backward kernels: the same ``alpha`` and output bit for bit, no
    ``[E]`` intermediates, and gradients to ``attn_l``, ``attn_r`` and ``fc`` summed in a fixed
    order that is another order than ``index_add``'s. The attention needs the CSRGraph's own
    edge order, so a DGL graph raises the ``TypeError`` of ``edge_weight=``.

    ``num_heads=H > 1`` is ``dglnn.GATConv(num_heads=H)``: ``fc`` maps to ``H * out_feats <=
    256``, ``attn_l`` / ``attn_r`` are ``(H, out_feats)``, the bias has ``H * out_feats`` entries
    and the result is ``[N, H, out_feats]``. MaxK keeps ``maxk`` features of the whole
    ``H * out_feats`` row; the attention is always the fused head-batched kernel and the
    aggregation the multi-head one (:mod:`maxk_kernels.heads`), which builds no plan.
    ``nonlinear="relu"`` is not implemented for ``H > 1``. The default ``num_heads=1`` is the
    single-head layer above, unchanged."""

    def __init__(self, in_feats, out_feats, maxk=32, negative_slope=0.2, attn_drop=0.,
                 feat_drop=0., bias=True, allow_zero_in_degree=False, topk_mode="exact",
                 nonlinear="maxk", fused_dropout=False, fused_attention=False, num_heads=1):
        super().__init__()
        self.num_heads = int(num_heads)
        if self.num_heads < 1:
            raise ValueError(f"num_heads must be >= 1, got {num_heads}")
        if self.num_heads > 1 and nonlinear == "relu":
            raise NotImplementedError('nonlinear="relu" with num_heads > 1: the dense multi-head '
                                      "aggregation is not implemented")
        if self.num_heads > 1 and self.num_heads * out_feats > 256:
            raise ValueError("num_heads * out_feats = D <= 256 (u8 selectors), got "
                             f"{self.num_heads * out_feats}")
        self.fused_dropout = bool(fused_dropout)
        self.fused_attention = bool(fused_attention)
        self.in_feats = in_feats
        self.out_feats = out_feats
        self.maxk = maxk
        self.negative_slope = float(negative_slope)
        self.attn_drop = float(attn_drop)
        self.feat_drop = float(feat_drop)
        self.allow_zero_in_degree = allow_zero_in_degree
        self.topk_mode = topk_mode
        self.nonlinear = _check_nonlinear(nonlinear)
        self.fc = nn.Linear(in_feats, self.num_heads * out_feats, bias=False)
        self.attn_l = nn.Parameter(torch.empty(self.num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(self.num_heads, out_feats))
        self.bias = nn.Parameter(torch.empty(self.num_heads * out_feats)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, graph, feat: torch.Tensor) -> torch.Tensor:
        _refuse_block(graph, "MaxKGATConv")
        csr = as_csr(graph, True)  # attention weights are an edge_weight: CSRGraph only
        if not self.allow_zero_in_degree and bool((csr.in_degrees() == 0).any()):
            raise ValueError("Graph has nodes with zero in-degree")
        h = self.fc(feat)
        if self.num_heads > 1:
            return self._forward_heads(csr, h)
        el = (h * self.attn_l).sum(-1)
        er = (h * self.attn_r).sum(-1)
        if self.fused_attention:
            alpha = gat_attention(csr, el, er, self.negative_slope)
        else:
            e = F.leaky_relu(el[csr.idx] + er[csr.edge_rows()], self.negative_slope)
            alpha = edge_softmax(csr, e)
        if self.attn_drop > 0:
            alpha = F.dropout(alpha, self.attn_drop, self.training)
        g = csr.with_values("sum")
        if self.nonlinear == "relu":
            x = F.dropout(h, self.feat_drop, self.training) if self.feat_drop > 0 else h
            rst = dense_aggregate(x, g, alpha)
        elif self.feat_drop > 0 and self.training and self.fused_dropout:
            rst = maxk_aggregate(h, g, self.maxk, self.topk_mode, dropout_p=self.feat_drop,
                                 edge_weight=alpha)
        elif self.feat_drop > 0 and self.training:
            sp_data, sp_index = maxk(h, self.maxk, self.topk_mode)
            sp_data = _sparse_dropout(sp_data, self.feat_drop, self.training)
            rst = spgemm(sp_data, sp_index, g, self.out_feats, edge_weight=alpha)
        else:
            rst = maxk_aggregate(h, g, self.maxk, self.topk_mode, edge_weight=alpha)
        if self.bias is not None:
            rst = rst + self.bias
        return rst

    def _forward_heads(self, csr: CSRGraph, h: torch.Tensor) -> torch.Tensor:
        """``num_heads = H > 1``: ``[N, H, out_feats]`` as ``dglnn.GATConv`` returns it. The scores
        are head-major ``[H, N]``, the attention is the head-batched fused kernel, MaxK keeps
        ``maxk`` of the whole ``H * out_feats`` row, and one multi-head aggregation weighs every
        kept feature by its own head's ``alpha``."""
        H, F_ = self.num_heads, self.out_feats
        hv = h.view(-1, H, F_)
        el = (hv * self.attn_l).sum(-1).t()
        er = (hv * self.attn_r).sum(-1).t()
        alpha = gat_attention_heads(csr, el, er, self.negative_slope)
        if self.attn_drop > 0:
            alpha = F.dropout(alpha, self.attn_drop, self.training)
        if self.feat_drop > 0 and self.training and not self.fused_dropout:
            sp_data, sp_index = maxk(h, self.maxk, self.topk_mode)
            sp_data = _sparse_dropout(sp_data, self.feat_drop, self.training)
            rst = heads_aggregate(csr, alpha, sp_data, sp_index, H * F_)
        else:
            rst = maxk_heads_aggregate(h, csr, alpha, self.maxk, self.topk_mode,
                                       dropout_p=self.feat_drop, training=self.training)
        if self.bias is not None:
            rst = rst + self.bias
        return rst.view(-1, H, F_)


class MaxKGINConv(nn.Module):
    """GIN layer (``dglnn.GINConv(learn_eps=True, activation=None)``, sum aggregator, no
    apply_func; utils/models.py:373) on MaxK features:
    ``rst = (1 + eps) x + sum_{u->v} x_u`` with ``x = feat_drop(MaxK(feat))`` through the
    SpGEMM kernels, or ``x = feat`` and the dense SpMM for ``nonlinear='relu'``."""

    def __init__(self, in_feats, out_feats=None, learn_eps=True, maxk=32, init_eps=0.,
                 topk_mode="exact", feat_drop=0., nonlinear="maxk", fused_dropout=False):
        super().__init__()
        self.fused_dropout = bool(fused_dropout)
        if out_feats is not None and out_feats != in_feats:
            raise ValueError("GINConv without apply_func keeps the feature size")
        self.in_feats = in_feats
        self.maxk = maxk
        self.topk_mode = topk_mode
        self.feat_drop = float(feat_drop)
        self.nonlinear = _check_nonlinear(nonlinear)
        eps = torch.tensor([float(init_eps)])
        if learn_eps:
            self.eps = nn.Parameter(eps)
        else:
            self.register_buffer("eps", eps)

    def forward(self, graph, feat: torch.Tensor, edge_weight=None) -> torch.Tensor:
        _refuse_block(graph, "MaxKGINConv")
        csr = as_csr(graph, edge_weight).with_values("sum")
        if self.nonlinear == "relu":
            x = F.dropout(feat, self.feat_drop, self.training) if self.feat_drop > 0 else feat
            return (1 + self.eps) * x + dense_aggregate(x, csr, edge_weight)
        x, neigh = _maxk_self_pair(self, feat, csr, edge_weight)
        return (1 + self.eps) * x + neigh


class MaxKSAGE(nn.Module):
    """utils/integrated_models.py:8-66 (MaxK applied inside each MaxKSAGEConv); with
    ``nonlinear='relu'`` the utils/models.py:109-165 SAGE: ReLU, then dglnn.SAGEConv(mean)."""

    def __init__(self, in_size, hid_size, num_hid_layers, out_size, maxk=32, feat_drop=0.5,
                 norm=False, nonlinear="maxk", fused_dropout=False, aggregator_type="mean"):
        super().__init__()
        self.nonlinear = _check_nonlinear(nonlinear)
        self.num_layers = num_hid_layers
        self.lin_in = nn.Linear(in_size, hid_size)
        self.lin_out = nn.Linear(hid_size, out_size)
        self.layers = nn.ModuleList(
            MaxKSAGEConv(hid_size, hid_size, aggregator_type, feat_drop=feat_drop,
                         norm=nn.LayerNorm(hid_size) if norm else None, maxk=maxk,
                         nonlinear=nonlinear, fused_dropout=fused_dropout)
            for _ in range(num_hid_layers))
        nn.init.xavier_uniform_(self.lin_in.weight)
        nn.init.xavier_uniform_(self.lin_out.weight)

    def forward(self, g, x, edge_weight=None):
        """``g``: a graph for every layer, or a list of sampled blocks, one per layer, outermost
        first (``NeighborSampler.sample``): ``x`` then holds the rows ``blocks[0].src_ids`` and
        the result the rows of the seeds."""
        blocks = list(g) if isinstance(g, (list, tuple)) else None
        if blocks is not None and len(blocks) != len(self.layers):
            raise ValueError(f"MaxKSAGE has {len(self.layers)} layers, got {len(blocks)} blocks")
        x = self.lin_in(x)
        for i, layer in enumerate(self.layers):
            if self.nonlinear == "relu":
                x = F.relu(x)
            x = layer(g if blocks is None else blocks[i], x, edge_weight)
        return self.lin_out(x)


class MaxKGCN(nn.Module):
    """utils/models.py:240-289 GCN (lin -> MaxK or ReLU -> dropout -> GraphConv(weight=None)
    -> LayerNorm)."""

    def __init__(self, in_size, hid_size, num_hid_layers, out_size, maxk=32, feat_drop=0.5,
                 norm=False, nonlinear="maxk", fused_dropout=False):
        super().__init__()
        self.nonlinear = _check_nonlinear(nonlinear)
        self.num_layers = num_hid_layers
        self.lin_in = nn.Linear(in_size, hid_size)
        self.lin_out = nn.Linear(hid_size, out_size)
        self.linlayers = nn.ModuleList(nn.Linear(hid_size, hid_size)
                                       for _ in range(num_hid_layers))
        self.gcnlayers = nn.ModuleList(MaxKGCNConv(hid_size, hid_size, weight=False, maxk=maxk,
                                                   allow_zero_in_degree=True,
                                                   feat_drop=feat_drop, nonlinear=nonlinear,
                                                   fused_dropout=fused_dropout)
                                       for _ in range(num_hid_layers))
        self.normlayers = nn.ModuleList(nn.LayerNorm(hid_size) for _ in range(num_hid_layers)
                                        ) if norm else None
        for lin in [self.lin_in, self.lin_out, *self.linlayers]:
            nn.init.xavier_uniform_(lin.weight)

    def forward(self, g, x, edge_weight=None):
        _refuse_block(g, "MaxKGCN")
        x = self.lin_in(x).relu()
        for i, conv in enumerate(self.gcnlayers):
            x = self.linlayers[i](x)
            if self.nonlinear == "relu":
                x = F.relu(x)
            x = conv(g, x, edge_weight)
            if self.normlayers is not None:
                x = self.normlayers[i](x)
        return self.lin_out(x)


class MaxKGIN(nn.Module):
    """utils/models.py:363-411 GIN (lin -> MaxK or ReLU -> dropout -> GINConv(learn_eps)
    -> LayerNorm), the constructor of utils/integrated_models.py:145-149."""

    def __init__(self, in_size, hid_size, num_hid_layers, out_size, maxk=32, feat_drop=0.5,
                 norm=False, nonlinear="maxk", fused_dropout=False):
        super().__init__()
        self.nonlinear = _check_nonlinear(nonlinear)
        self.num_layers = num_hid_layers
        self.lin_in = nn.Linear(in_size, hid_size)
        self.lin_out = nn.Linear(hid_size, out_size)
        self.linlayers = nn.ModuleList(nn.Linear(hid_size, hid_size)
                                       for _ in range(num_hid_layers))
        self.ginlayers = nn.ModuleList(MaxKGINConv(hid_size, maxk=maxk, feat_drop=feat_drop,
                                                   nonlinear=nonlinear,
                                                   fused_dropout=fused_dropout)
                                       for _ in range(num_hid_layers))
        self.normlayers = nn.ModuleList(nn.LayerNorm(hid_size) for _ in range(num_hid_layers)
                                        ) if norm else None
        for lin in [self.lin_in, self.lin_out, *self.linlayers]:
            nn.init.xavier_uniform_(lin.weight)

    def forward(self, g, x, edge_weight=None):
        _refuse_block(g, "MaxKGIN")
        x = self.lin_in(x).relu()
        for i, conv in enumerate(self.ginlayers):
            x = self.linlayers[i](x)
            if self.nonlinear == "relu":
                x = F.relu(x)
            x = conv(g, x, edge_weight)
            if self.normlayers is not None:
                x = self.normlayers[i](x)
        return self.lin_out(x)
