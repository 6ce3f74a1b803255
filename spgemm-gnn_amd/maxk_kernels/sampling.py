"""Neighbour sampling on the device: sampled blocks, and the MaxK aggregation on them.

* :func:`sample_neighbors` draws at most ``fanout`` in-edges per seed row without replacement
  (``maxk_sample_neighbors``: the ``fanout`` edges of lowest rank under a counter-based hash of
  ``(seed, edge)``, so a row's sample depends on neither the batch nor the row's place in it).
* :func:`block_compact` relabels the sampled columns: the seeds first, then every other column
  once in ascending order (``maxk_block_compact``).
* :class:`Block` is the rectangular :class:`~maxk_kernels.CSRGraph` the two produce: ``num_dst``
  rows over ``num_src`` columns, the destination nodes being the first ``num_dst`` source nodes
  (DGL's block convention), with ``src_ids`` / ``dst_ids`` / ``eids`` into the parent graph.
* :class:`NeighborSampler` samples one block per layer, outermost first, with the return value
  of ``dgl.dataloading.NeighborSampler.sample``.
* :func:`block_aggregate` / :func:`block_self_aggregate`: ``MaxKFunction`` on the ``num_src``
  input rows, then the plan-less weighted sum of the multi-head aggregation at one head
  (``HeadsAggregateFunction`` with ``alpha = block.val[None]``). A block lives for one step, where
  a plan's sorts would never pay back. ``D % 4 == 0`` and ``k <= D <= 256`` (that kernel's limit).

The backward needs the block's transposed structure: ``ops.csr_transpose`` per block.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .autograd import CSRGraph, densify, maxk
from .heads import HeadsAggregateFunction

_MASK64 = 0xFFFFFFFFFFFFFFFF


def sample_neighbors(graph: CSRGraph, seeds: torch.Tensor, fanout: int, seed: int
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ptr int32 [S + 1], col int32 [M], eid int32 [M])``: the sampled in-edges of the rows
    ``seeds`` (int32, on the graph's device), ``col`` the global column and ``eid`` the edge
    number in ``graph``, ``M = ptr[S]``. ``fanout < 0`` keeps every neighbour. The slicing to
    ``M`` costs one read-back of ``ptr[S]`` (a stream synchronisation); ``ops.sample_neighbors``
    returns the whole buffers without one."""
    out_ptr, col, eid = ops.sample_neighbors(graph.ptr, graph.idx, seeds, fanout, seed)
    m = int(out_ptr[-1])
    if m > col.numel():
        raise ValueError(f"the sample holds {m} edges but the bound for distinct seeds is "
                         f"{col.numel()}: seeds repeat")
    return out_ptr, col[:m], eid[:m]


def block_compact(seeds: torch.Tensor, cols: torch.Tensor, num_cols: int
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(src_ids int32 [num_src], local_col int32 [M])``: the seeds in their order, then every
    other column of ``cols`` once, ascending; ``src_ids[local_col] == cols``. Reads the count pair
    back (one synchronisation) and raises ``ValueError`` when the seeds are not distinct."""
    src_ids, local_col, counts = ops.block_compact(seeds, cols, num_cols)
    num_src, distinct = (int(v) for v in counts.tolist())
    if distinct != seeds.numel():
        raise ValueError(f"seeds must be distinct: {seeds.numel()} seeds name {distinct} nodes")
    return src_ids[:num_src], local_col


@dataclass
class Block(CSRGraph):
    """A sampled bipartite block: row ``r`` (destination ``dst_ids[r]``) aggregates from the
    local columns ``idx[ptr[r]:ptr[r+1]]``, which index ``src_ids``. ``num_nodes`` is the row
    count ``num_dst``; everything sized by columns (``out_degrees``, the transposed structure,
    the plan) uses ``num_src``. ``val`` holds the parent's edge values gathered through ``eids``
    (ones without a parent); ``in_degrees``, ``edge_values`` and ``with_values`` are over the
    sampled edges, so ``with_values("mean")`` is DGL's mean over a block."""

    num_src: int = 0
    src_ids: Optional[torch.Tensor] = None
    eids: Optional[torch.Tensor] = None

    def __post_init__(self):
        super().__post_init__()
        self.num_src = int(self.num_src)

    @property
    def num_dst(self) -> int:
        return self.num_nodes

    @property
    def dst_ids(self) -> Optional[torch.Tensor]:
        return None if self.src_ids is None else self.src_ids[:self.num_dst]

    def plan(self, dim_origin: int, dim_k: int) -> ops.GraphPlan:
        key = ("plan", int(dim_origin), int(dim_k))
        plan = self._values.get(key)
        if plan is None:
            plan = ops.GraphPlan(self.ptr, self.idx, self.val, self.num_dst, self.num_edges,
                                 int(dim_origin), int(dim_k), num_cols=self.num_src)
            self._values[key] = plan
        return plan

    def weighted_plan(self, dim_origin: int, dim_k: int) -> ops.GraphPlan:
        raise NotImplementedError("edge_weight on a Block is not implemented: block_aggregate "
                                  "and block_self_aggregate take the block's own values")

    def _num_cols(self) -> int:
        return self.num_src

    def _transposed_graph(self, ptr_t, idx_t, val_t) -> "Block":
        """A^T, ``num_src`` rows over ``num_dst`` columns."""
        return Block(ptr_t, idx_t, val_t, num_src=self.num_dst)

    def with_values(self, kind: str) -> "Block":
        key = ("graph", kind)
        g = self._values.get(key)
        if g is None:
            g = Block(self.ptr, self.idx, self.edge_values(kind), num_src=self.num_src,
                      src_ids=self.src_ids, eids=self.eids)
            g._values["edge_rows"] = self.edge_rows()
            if "transposed_structure" in self._values:
                g._values["transposed_structure"] = self._values["transposed_structure"]
            self._values[key] = g
        return g


def to_block(graph: CSRGraph, seeds: torch.Tensor, fanout: int, seed: int) -> Block:
    """One layer's block: :func:`sample_neighbors` of ``seeds`` on ``graph``, then
    :func:`block_compact` (two read-backs). ``graph`` may itself be rectangular (a ``Block``)."""
    num_cols = graph.num_src if isinstance(graph, Block) else graph.num_nodes
    out_ptr, col, eid = sample_neighbors(graph, seeds, fanout, seed)
    src_ids, local_col = block_compact(seeds, col, num_cols)
    return Block(out_ptr, local_col, graph.val[eid.to(torch.int64)], num_src=src_ids.numel(),
                 src_ids=src_ids, eids=eid)


def _fmix64(x: int) -> int:
    x &= _MASK64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _MASK64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _MASK64
    return x ^ (x >> 33)


def layer_seed(seed: int, call: int, layer: int) -> int:
    """The sampler seed of layer ``layer`` in call ``call`` of a :class:`NeighborSampler`:
    ``fmix64(fmix64(seed + 0x9E3779B97F4A7C15 * (call + 1)) + layer)`` with fmix64 the murmur3
    64-bit finaliser (``x ^= x >> 33; x *= 0xFF51AFD7ED558CCD; x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53; x ^= x >> 33``), all arithmetic modulo 2^64."""
    return _fmix64(_fmix64(int(seed) + 0x9E3779B97F4A7C15 * (int(call) + 1)) + int(layer))


class NeighborSampler:
    """``NeighborSampler(fanouts, seed).sample(graph, seeds) -> (input_ids, output_ids,
    blocks)``, the contract of ``dgl.dataloading.NeighborSampler``: ``fanouts[l]`` neighbours for
    layer ``l`` (``-1``: all), ``blocks[l]`` the block layer ``l`` of the model consumes,
    outermost (the one that reads the input features) first. The blocks are sampled from the
    output layer inwards: the seeds of each inner layer are the ``src_ids`` of the layer after
    it. ``input_ids = blocks[0].src_ids`` and ``output_ids = seeds`` are global node ids.

    Layer ``l`` of the ``c``-th call to :meth:`sample` (``c`` counts from 0 and is kept in
    ``self.calls``) draws with :func:`layer_seed` ``(seed, c, l)``, so a sampler built with the
    same seed replays the same blocks, and no two layers or calls share their random numbers."""

    def __init__(self, fanouts: Sequence[int], seed: int = 0):
        self.fanouts = [int(f) for f in fanouts]
        if not self.fanouts or any(f == 0 for f in self.fanouts):
            raise ValueError("fanouts must be a non-empty list of positive fanouts (or -1)")
        self.seed = int(seed)
        self.calls = 0

    def sample(self, graph: CSRGraph, seeds: torch.Tensor):
        if not isinstance(graph, CSRGraph):
            raise TypeError("graph must be a maxk_kernels.CSRGraph")
        seeds = seeds.to(device=graph.device, dtype=torch.int32).contiguous()
        call, self.calls = self.calls, self.calls + 1
        blocks: List[Block] = []
        cur = seeds
        for layer in reversed(range(len(self.fanouts))):
            block = to_block(graph, cur, self.fanouts[layer], layer_seed(self.seed, call, layer))
            blocks.insert(0, block)
            cur = block.src_ids
        return cur, seeds, blocks


def _check_block(x: torch.Tensor, block: Block, k: int) -> None:
    if not isinstance(block, Block):
        raise TypeError("block must be a maxk_kernels.Block")
    if block.num_src < block.num_dst:
        raise ValueError("a block's destination nodes are its first source nodes: "
                         f"num_src = {block.num_src} < num_dst = {block.num_dst}")
    if x.dim() != 2 or x.shape[0] != block.num_src:
        raise RuntimeError(f"x must be [num_src, D] = [{block.num_src}, D], got "
                           f"{tuple(x.shape)}")
    d = x.shape[1]
    if d % 4 != 0 or not 1 <= k <= d <= 256:
        raise RuntimeError("the block aggregation needs D % 4 == 0 and k <= D <= 256, got "
                           f"D = {d}, k = {k}")


def block_spgemm(sp_data: torch.Tensor, sp_index: torch.Tensor, block: Block,
                 dim_origin: int) -> torch.Tensor:
    """``A_block @ densify(sp_data, sp_index)`` as f32 ``[num_dst, D]`` from CBSR tables of
    ``num_src`` rows, differentiable in ``sp_data``: the aggregation step of
    :func:`block_aggregate` on tables the caller already holds."""
    return HeadsAggregateFunction.apply(block, block.val[None], sp_data, sp_index,
                                        int(dim_origin))


def block_aggregate(x: torch.Tensor, block: Block, k: int, mode: str = "exact",
                    dropout_p: float = 0.0, training: bool = True,
                    seed: Optional[int] = None) -> torch.Tensor:
    """``A_block @ densify(MaxK(x))`` as f32 ``[num_dst, D]`` from ``x [num_src, D]``,
    differentiable in ``x``; the weights are ``block.val`` (``block.with_values("mean")`` for a
    mean). ``dropout_p``, ``training``, ``seed`` as for :func:`maxk_kernels.maxk`."""
    _check_block(x, block, int(k))
    sp_data, sp_index = maxk(x, k, mode, dropout_p=dropout_p, training=training, seed=seed)
    return block_spgemm(sp_data, sp_index, block, x.shape[1])


def block_self_aggregate(x: torch.Tensor, block: Block, k: int, mode: str = "exact",
                         dropout_p: float = 0.0, training: bool = True,
                         seed: Optional[int] = None):
    """``(x_masked [num_src, D], agg [num_dst, D])``: the dense masked input
    ``dropout(x * topk_mask(x))`` and its aggregation over the block, both differentiable in
    ``x``. The self term of a layer is ``x_masked[:block.num_dst]``."""
    _check_block(x, block, int(k))
    sp_data, sp_index = maxk(x, k, mode, dropout_p=dropout_p, training=training, seed=seed)
    agg = block_spgemm(sp_data, sp_index, block, x.shape[1])
    return densify(sp_data, sp_index, x.shape[1]), agg
