"""maxk_kernels — MI355X-native drop-in for the reference's ``maxk_kernels`` extension.

``import maxk_kernels`` exposes the reference's four bound functions with the same
positional signatures:

    maxk_forward(input, k) -> sp_data [N, k]
    maxk_backward(grad_output, indices) -> [N, D]
    spgemm_forward(ptr, idx, val, sp_data, sp_index, num_nodes, num_edges, dim_k, dim_origin)
        -> (out [N, D], sp_index)
    spgemm_backward(ptr, idx, val, grad_output, sp_index, num_nodes, num_edges, dim_k,
                    dim_origin) -> grad_sp [N, k]

all running hand-written gfx950 HIP kernels through the C ABI of include/maxk_hip.h
(libmaxk_hip.so). There is no fallback: if the library is missing the import fails.
"""
from ._lib import LIB_PATH, MaxKError, lib  # noqa: F401  (loads libmaxk_hip.so)
from .ops import (  # noqa: F401
    TOPK_MODES,
    GraphPlan,
    cbsr_stats,
    csr_transpose,
    clear_plan_cache,
    dense_spmm,
    edge_softmax_backward,
    edge_softmax_row_limits,
    get_plan,
    heads_row_limits,
    max_row_limits,
    maxk_backward,
    maxk_forward,
    plan_col_order,
    sample_row_limits,
    spgemm_backward,
    spgemm_edge_grad,
    spgemm_forward,
    subgraph_row_limits,
    transpose_digit_bits,
)
from .autograd import (  # noqa: F401
    CSRGraph,
    DenseAggFunction,
    DenseEdgeWeightedFunction,
    EdgeSoftmaxFunction,
    EdgeWeightedFunction,
    MaxKAggregateFunction,
    MaxKFunction,
    MaxKSelfAggregateFunction,
    SpGEMMFunction,
    dense_aggregate,
    densify,
    edge_softmax,
    maxk,
    maxk_aggregate,
    maxk_self_aggregate,
    spgemm,
)

from . import torch_ops  # noqa: F401,E402  (registers torch.ops.maxk.*)
from .attention import GATAttentionFunction, gat_attention  # noqa: F401,E402  (and its operators)
from .heads import (  # noqa: F401,E402  (and its operators)
    GATAttentionHeadsFunction,
    HeadsAggregateFunction,
    gat_attention_heads,
    heads_aggregate,
    maxk_heads_aggregate,
)
from .pooling import (  # noqa: F401,E402  (and its operators)
    MaxAggregateFunction,
    dense_max_aggregate,
    max_aggregate,
    maxk_max_aggregate,
)
from .sampling import (  # noqa: F401,E402
    Block,
    NeighborSampler,
    block_aggregate,
    block_compact,
    block_self_aggregate,
    block_spgemm,
    layer_seed,
    sample_neighbors,
    to_block,
)
from .subgraph import (  # noqa: F401,E402
    ClusterLoader,
    Subgraph,
    node_subgraph,
    random_partition,
)
from .layers import (  # noqa: F401,E402
    MaxKGCN,
    MaxKGATConv,
    MaxKGCNConv,
    MaxKGIN,
    MaxKGINConv,
    MaxKSAGE,
    MaxKSAGEConv,
)

__all__ = [
    "maxk_forward", "maxk_backward", "spgemm_forward", "spgemm_backward",
    "dense_spmm", "cbsr_stats", "plan_col_order", "GraphPlan", "get_plan", "clear_plan_cache", "CSRGraph",
    "MaxKFunction", "MaxKAggregateFunction", "SpGEMMFunction", "maxk", "spgemm", "maxk_aggregate", "MaxKError",
    "densify", "MaxKSAGEConv", "MaxKGCNConv", "MaxKGINConv", "MaxKSAGE", "MaxKGCN",
    "MaxKGIN", "dense_aggregate", "DenseAggFunction", "MaxKSelfAggregateFunction",
    "maxk_self_aggregate", "spgemm_edge_grad", "EdgeWeightedFunction", "DenseEdgeWeightedFunction",
    "edge_softmax", "edge_softmax_backward", "edge_softmax_row_limits", "EdgeSoftmaxFunction",
    "MaxKGATConv", "gat_attention", "GATAttentionFunction",
    "gat_attention_heads", "GATAttentionHeadsFunction", "heads_aggregate", "maxk_heads_aggregate",
    "HeadsAggregateFunction", "heads_row_limits",
    "max_aggregate", "maxk_max_aggregate", "dense_max_aggregate", "MaxAggregateFunction",
    "max_row_limits",
    "sample_neighbors", "block_compact", "Block", "to_block", "NeighborSampler", "layer_seed",
    "block_aggregate", "block_self_aggregate", "block_spgemm", "sample_row_limits",
    "node_subgraph", "Subgraph", "random_partition", "ClusterLoader", "subgraph_row_limits",
    "csr_transpose", "transpose_digit_bits",
]

ABI_VERSION = lib.maxk_abi_version()
