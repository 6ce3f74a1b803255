"""Induced subgraphs on the device, and mini-batches of clusters.

* :func:`node_subgraph` extracts ``A[nodes][:, nodes]`` (``maxk_induced_subgraph_count`` /
  ``_fill``: one int32 mark per node gives the local numbering, rows are compacted by ballots in
  edge order), the result of ``dgl.node_subgraph``.
* :class:`Subgraph` is the square :class:`~maxk_kernels.CSRGraph` it produces, with ``node_ids``
  and ``eids`` into the parent. Every layer, aggregator, model and ``edge_weight=`` path takes it
  as it takes any ``CSRGraph``; its plans are kept on the object.
* :func:`random_partition` is the built-in partition; any part id per node serves.
* :class:`ClusterLoader` yields one :class:`Subgraph` per batch of clusters, with the edges
  between the clusters of a batch (Cluster-GCN). With a fixed partition the same subgraphs come
  back every epoch, so the loader keeps them, and with them the plans, transposed structures and
  edge values the layers built on them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import ops
from .autograd import CSRGraph
from .sampling import Block, layer_seed


@dataclass
class Subgraph(CSRGraph):
    """The induced subgraph of ``node_ids`` in a parent graph of ``parent_num_nodes`` nodes: row
    ``i`` is node ``node_ids[i]`` of the parent and keeps the in-edges whose source is selected
    too, in the parent's order; ``idx`` holds positions in ``node_ids``; edge ``j`` is edge
    ``eids[j]`` of the parent, and ``val`` the parent's values gathered through ``eids``.

    ``in_degrees``, ``out_degrees`` and ``edge_values`` are the inherited ones: they are computed
    over the subgraph's own edges, so ``with_values("mean")`` or ``"both"`` normalise by the
    degrees inside the subgraph. That is ``dgl.node_subgraph`` followed by a layer, and the
    normalisation of Cluster-GCN. :meth:`plan` keeps its plans on the object (as ``Block.plan``
    does) instead of the global cache of 32 plans: a loader with more parts than that would evict
    its own clusters every epoch. A plan is rebuilt after an in-place edit of ``ptr`` or ``idx``
    that torch's version counter shows and value-refreshed after one of ``val``, as
    ``ops.get_plan`` does. :meth:`with_values` is overridden only to return a ``Subgraph`` (the
    same inherited values on the same structure, with ``node_ids`` / ``eids`` carried along), so
    that the plans of the graph a layer computes on stay on an object the subgraph owns."""

    node_ids: Optional[torch.Tensor] = None
    eids: Optional[torch.Tensor] = None
    parent_num_nodes: int = 0

    def __post_init__(self):
        super().__post_init__()
        self.parent_num_nodes = int(self.parent_num_nodes)

    def edge_data(self, t: torch.Tensor) -> torch.Tensor:
        """``t[eids]``: the subgraph's rows of a per-edge tensor of the parent, such as the
        ``edge_weight`` of a layer (differentiable in ``t``)."""
        return t[self.eids.to(torch.int64)]

    def plan(self, dim_origin: int, dim_k: int) -> ops.GraphPlan:
        key = ("plan", int(dim_origin), int(dim_k))
        structure = (ops._version(self.ptr), ops._version(self.idx))
        plan, built_for = self._values.get(key, (None, None))
        if plan is None or built_for != structure:   # an in-place edit of ptr or idx: rebuild
            plan = ops.GraphPlan(self.ptr, self.idx, self.val, self.num_nodes, self.num_edges,
                                 int(dim_origin), int(dim_k))
            self._values[key] = (plan, structure)
        elif ops._values_stale(plan, self.val):
            plan.refresh_values(self.val)
        return plan

    def with_values(self, kind: str) -> "Subgraph":
        key = ("graph", kind)
        g = self._values.get(key)
        if g is None:
            g = Subgraph(self.ptr, self.idx, self.edge_values(kind), node_ids=self.node_ids,
                         eids=self.eids, parent_num_nodes=self.parent_num_nodes)
            g._values["edge_rows"] = self.edge_rows()
            if "transposed_structure" in self._values:
                g._values["transposed_structure"] = self._values["transposed_structure"]
            self._values[key] = g
        return g


def node_subgraph(graph: CSRGraph, nodes: torch.Tensor) -> Subgraph:
    """The induced subgraph of ``nodes`` (distinct node ids of ``graph``, in the order that
    becomes the subgraph's numbering). Two launches' worth of kernels and one read-back between
    them: the number of kept edges sizes the result. ``ValueError`` for repeated or out-of-range
    nodes, ``TypeError`` for a ``Block`` (it is rectangular)."""
    if isinstance(graph, Block):
        raise TypeError("node_subgraph needs a square CSRGraph: a Block is rectangular, its rows "
                        "and columns are numbered apart")
    if not isinstance(graph, CSRGraph):
        raise TypeError("graph must be a maxk_kernels.CSRGraph")
    if nodes.is_floating_point() or nodes.is_complex() or nodes.dtype == torch.bool:
        raise TypeError(f"nodes must hold integer node ids, got {nodes.dtype}")
    n = graph.num_nodes
    if nodes.dtype != torch.int32:
        # out of range on the given dtype stays out of range after narrowing (an int64 id of
        # 2^32 + 5 must not wrap to 5): -1 and n are both outside [0, n), and the kernel counts
        # them
        nodes = nodes.clamp(min=-1, max=n)
    nodes = nodes.to(device=graph.device, dtype=torch.int32).contiguous()
    s = nodes.numel()
    scratch = torch.empty(ops.induced_subgraph_scratch_bytes(n, s), dtype=torch.uint8,
                          device=graph.device)
    out_ptr, counts = ops.induced_subgraph_count(graph.ptr, graph.idx, nodes, scratch=scratch)
    m, distinct, stray = (int(v) for v in counts.tolist())
    if stray:
        raise ValueError(f"{stray} of the {s} nodes lie outside [0, {n})")
    if distinct != s:
        raise ValueError(f"nodes must be distinct: {s} entries name {distinct} nodes")
    col, eid = ops.induced_subgraph_fill(graph.ptr, graph.idx, nodes, out_ptr, capacity=m,
                                         scratch=scratch)
    return Subgraph(out_ptr, col, graph.val[eid.to(torch.int64)], node_ids=nodes, eids=eid,
                    parent_num_nodes=n)


def random_partition(num_nodes: int, num_parts: int, seed: int = 0) -> torch.Tensor:
    """A part id per node, int32 ``[num_nodes]`` on the CPU, deterministic in its arguments:
    with ``perm = torch.randperm(num_nodes, generator=torch.Generator().manual_seed(seed))``,
    node ``perm[j]`` is in part ``j * num_parts // num_nodes``. Part sizes differ by at most 1."""
    num_nodes, num_parts = int(num_nodes), int(num_parts)
    if not 1 <= num_parts <= max(num_nodes, 1):
        raise ValueError(f"num_parts must be in [1, num_nodes], got {num_parts} for "
                         f"{num_nodes} nodes")
    perm = torch.randperm(num_nodes, generator=torch.Generator().manual_seed(int(seed)))
    parts = torch.empty(num_nodes, dtype=torch.int32)
    parts[perm] = (torch.arange(num_nodes, dtype=torch.int64) * num_parts // max(num_nodes, 1)
                   ).to(torch.int32)
    return parts


class ClusterLoader:
    """``for sub in ClusterLoader(graph, parts, clusters_per_batch): model(sub,
    x[sub.node_ids.long()])``: the batches of Cluster-GCN.

    ``parts`` is a part id in ``[0, P)`` per node (``P = parts.max() + 1``, every part
    non-empty), or an int ``P`` for :func:`random_partition` ``(num_nodes, P, seed)``. An epoch
    (one iteration over the loader) has ``len(loader) = ceil(P / clusters_per_batch)`` batches.
    Batch ``b`` takes the clusters ``order[b * clusters_per_batch : (b + 1) *
    clusters_per_batch]`` and yields the induced subgraph of their union, the edges between the
    clusters included, with ``node_ids`` ascending (so one batch of all clusters is the graph
    itself). ``order`` is ``0 .. P - 1`` without ``shuffle``; with it, epoch ``e`` (counted from
    0 in ``self.epoch``) draws ``torch.randperm(P, generator=torch.Generator().manual_seed(
    layer_seed(seed, e, 0)))``.

    ``cache``: keep every :class:`Subgraph` after its first build, keyed by its set of clusters,
    with whatever plans and transposed structure the layers hung on it. The default keeps them
    when the batches recur (no ``shuffle``, or ``clusters_per_batch == 1``) and nothing
    otherwise."""

    def __init__(self, graph: CSRGraph, parts: Union[int, torch.Tensor],
                 clusters_per_batch: int = 1, shuffle: bool = False, seed: int = 0,
                 cache: Optional[bool] = None):
        if isinstance(graph, Block) or not isinstance(graph, CSRGraph):
            raise TypeError("graph must be a square maxk_kernels.CSRGraph")
        self.graph = graph
        self.clusters_per_batch = int(clusters_per_batch)
        if self.clusters_per_batch < 1:
            raise ValueError(f"clusters_per_batch must be at least 1, got {clusters_per_batch}")
        self.shuffle, self.seed, self.epoch = bool(shuffle), int(seed), 0
        n = graph.num_nodes
        if isinstance(parts, int):
            parts = random_partition(n, parts, self.seed)
        parts = torch.as_tensor(parts).detach().cpu()
        if parts.dim() != 1 or parts.numel() != n or parts.is_floating_point():
            raise ValueError(f"parts must hold one integer part id per node, [{n}]")
        parts = parts.to(torch.int64)
        if n == 0 or int(parts.min()) < 0:
            raise ValueError("part ids must lie in [0, P): the graph has no nodes, or an id is "
                             "negative")
        self.num_parts = int(parts.max()) + 1
        sizes = torch.bincount(parts, minlength=self.num_parts)
        if int(sizes.min()) == 0:
            empty = torch.nonzero(sizes == 0).flatten().tolist()
            raise ValueError(f"empty parts: {empty[:8]} of [0, {self.num_parts}) have no node")
        self.parts = parts.to(torch.int32)
        order = torch.argsort(parts, stable=True).to(torch.int32)    # ascending inside a part
        self._members: List[torch.Tensor] = [m.to(graph.device)
                                             for m in torch.split(order, sizes.tolist())]
        self.cache = (not self.shuffle or self.clusters_per_batch == 1) if cache is None \
            else bool(cache)
        self._subgraphs: Dict[Tuple[int, ...], Subgraph] = {}

    def __len__(self) -> int:
        return -(-self.num_parts // self.clusters_per_batch)

    def batches(self, epoch: int) -> List[Tuple[int, ...]]:
        """The clusters of every batch of epoch ``epoch``, each ascending."""
        if self.shuffle:
            gen = torch.Generator().manual_seed(layer_seed(self.seed, int(epoch), 0))
            order = torch.randperm(self.num_parts, generator=gen).tolist()
        else:
            order = list(range(self.num_parts))
        c = self.clusters_per_batch
        return [tuple(sorted(order[b:b + c])) for b in range(0, self.num_parts, c)]

    def subgraph(self, clusters: Tuple[int, ...]) -> Subgraph:
        """The induced subgraph of the union of ``clusters``."""
        key = tuple(sorted(int(c) for c in clusters))
        sub = self._subgraphs.get(key) if self.cache else None
        if sub is None:
            nodes = self._members[key[0]] if len(key) == 1 else \
                torch.sort(torch.cat([self._members[c] for c in key])).values
            sub = node_subgraph(self.graph, nodes)
            if self.cache:
                self._subgraphs[key] = sub
        return sub

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        for clusters in self.batches(epoch):
            yield self.subgraph(clusters)
