"""The four functions of the reference's ``maxk_kernels`` extension, on the gfx950 C ABI.

Reference binding: pybind11 module ``maxk_kernels`` (PyInit SO@0xfc90) with the wrappers
``maxk_forward`` (SO@0xe340), ``maxk_backward`` (SO@0xe690), ``spgemm_forward``
(SO@0xea20) and ``spgemm_backward`` (SO@0xf170); argument checks recovered from
``kernels/maxk_bindings.cpp`` lines 27-30, 34-36, 45-54, 65-71.

Same names, same positional signatures, same return shapes and the same RuntimeError
messages for the same checks. Differences (all fixes of SURVEY §8(b) defects):

* kernels are launched on the current HIP stream with no device-wide synchronisation;
* ``spgemm_forward/backward`` derive their partition metadata from ``ptr`` (cached per
  graph) instead of reading ``../w12_nz64_warp_4/graph.warp4`` and printing to stdout;
* ``maxk_backward`` returns a stable ``[N, D]`` shape when ``dim_origin`` is given;
* ``maxk_forward`` can also return ``sp_index`` (the reference computes and drops it).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import os
import threading
from typing import Optional, Tuple

import torch

from ._lib import ACC_KINDS, BWD_ALGOS, COL_ORDERS, PlanInfo, PlanOptions, check, lib

TOPK_MODES = {"exact": 0, "ref_compat": 1}


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


_SAME_DEVICE = contextlib.nullcontext()


def _device(dev: torch.device):
    """``torch.cuda.device(dev)``, or a no-op when ``dev`` is already current (host cost)."""
    return _SAME_DEVICE if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def _version(t: Optional[torch.Tensor]) -> int:
    """``t._version``, or 0 for a tensor made under ``torch.inference_mode()``: such a tensor
    tracks no version counter (reading it raises) and cannot be edited in place outside
    inference mode, so there is no edit to see."""
    if t is None:
        return -1
    try:
        return t._version
    except RuntimeError:  # "Inference tensors do not track version counter."
        return 0


def _need(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(msg)


def _refuse_capture(what: str, remedy: str) -> None:
    """Raises while the current stream is being captured into a graph, before any launch, event
    or allocation: for the calls whose host-side work (a plan build, a value refresh, a drawn
    seed) a replay would silently skip. Not used on the compute path, which costs no query."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} cannot run while a graph is being captured: {remedy}")


def _check_tensor(t: torch.Tensor, name: str, dtype: Optional[torch.dtype] = None) -> None:
    _need(isinstance(t, torch.Tensor), f"{name} must be a tensor")
    _need(t.is_cuda, f"{name} must be a CUDA tensor")
    _need(t.is_contiguous(), f"{name} must be contiguous")
    if dtype is not None:
        _need(t.dtype == dtype, f"{name} must be {str(dtype).replace('torch.', '')}")


def _check_ptr(ptr, name: str, count: str) -> None:
    """A row-pointer array: int32, one entry more than the ``count`` it is named after."""
    _check_tensor(ptr, name, torch.int32)
    _need(ptr.dim() == 1 and ptr.numel() >= 1, f"{name} must have {count}+1 entries")


def _table(t: torch.Tensor, name: str, dtype: torch.dtype, rows: int, k: int) -> int:
    """A [rows, k] CBSR table whose rows may be strided (interleaved records): returns the row
    stride in elements."""
    _need(isinstance(t, torch.Tensor) and t.is_cuda, f"{name} must be a CUDA tensor")
    _need(t.dtype == dtype, f"{name} must be {str(dtype).replace('torch.', '')}")
    _need(t.dim() == 2 and tuple(t.shape) == (rows, k), f"{name} must be [{rows}, {k}]")
    _need(t.stride(1) == 1 and (rows <= 1 or t.stride(0) >= k),
          f"{name} must have unit column stride and row stride >= k")
    return t.stride(0) if rows > 1 else k


def _rows_in_place(t: torch.Tensor) -> torch.Tensor:
    """``t`` if :func:`_table` takes its rows as they are (2-D, unit column stride, row stride >=
    the width; one row: any row stride), else a contiguous copy."""
    if t.dim() != 2 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t.contiguous()
    return t


def _records(buf, layout, rows: int, k: int, name: str) -> int:
    """A u8 [rows, record_bytes] buffer of forward records in chunk layout ``layout`` (1, 2 or
    4, ``maxk_plan_info.fwd_layout``); rows may be strided: returns the row stride in bytes."""
    _need(isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.uint8 and
          buf.dim() == 2 and buf.shape[0] == rows, f"{name} must be a u8 [{rows}, bytes] CUDA tensor")
    used = {1: 5 * k, 2: 16 * ((k + 2) // 3), 4: 16 * (k // 2)}.get(int(layout), 0)
    _need(buf.shape[1] >= used, f"{name} rows must hold {used} bytes")
    _need(rows <= 1 or (buf.stride(1) == 1 and buf.stride(0) >= buf.shape[1]),
          f"{name} must have unit column stride and row stride >= its width")
    return buf.stride(0) if rows > 1 else buf.shape[1]


def _dropout_arg(dropout):
    """``dropout`` of :func:`maxk_forward` / :func:`maxk_backward` as ``(p, seed, row_offset)``
    with the seed taken modulo 2^64, or ``None`` when there is nothing to drop (``None`` or
    ``p == 0``: the path without dropout, unchanged)."""
    if dropout is None:
        return None
    _need(isinstance(dropout, (tuple, list)) and len(dropout) in (2, 3),
          "dropout must be (p, seed) or (p, seed, row_offset)")
    p, seed = float(dropout[0]), int(dropout[1]) & 0xFFFFFFFFFFFFFFFF
    row_offset = int(dropout[2]) if len(dropout) == 3 else 0
    if p == 0.0 and row_offset >= 0:
        return None
    return p, seed, row_offset


# -------------------------------------------------------------------------------------
# MaxK top-k
# -------------------------------------------------------------------------------------
def maxk_forward(input: torch.Tensor, k: int, mode: str = "exact",
                 return_index: bool = False, out=None, return_count: bool = False,
                 stats: Optional[torch.Tensor] = None, records=None,
                 return_values: bool = True, dropout=None, dense=None):
    """MaxK nonlinearity -> CBSR. Reference: ``maxk_forward(input, k) -> [N, k] f32``.

    Checks (bindings.cpp:27-30): "input must be a CUDA tensor", "input must be
    contiguous", "Input must be 2D tensor", "k must be between 1 and input dimension".
    ``mode='exact'`` selects the true top-k (utils/models.py:14 semantics), ``'ref_compat'``
    the reference kernel's 8-step bisection, bit-exact. With ``return_index=True`` returns
    ``(sp_data, sp_index)`` with ``sp_index`` u8 ``[N, k]`` in ascending feature order.
    ``out=(sp_data, sp_index)`` writes into caller-owned ``[N, k]`` tables with unit column
    stride (rows may be strided: the interleaved send records of
    :class:`maxk_kernels.dist.ShardedAggregation`). ``return_count=True``
    appends the int32 ``[N]`` number of filled slots per row (``k`` in exact mode; in
    ref_compat mode the slots past it are the reference's ``(0.0f, 0)`` padding).
    ``stats``: a contiguous int32 CUDA tensor of 2 elements (e.g. a view into a record) that
    receives the fixed-point statistics of the emitted table with the top-k
    (``maxk_topk_cbsr_ex``; its scratch comes from torch's caching allocator): the pair
    :meth:`GraphPlan.forward` takes as ``stats=stats.view(1, 2)`` instead of its own pass over
    the table.
    ``records=(buf, layout)``: the top-k also writes each row's forward record into ``buf``,
    a u8 ``[N, record_bytes]`` CUDA tensor, in the chunk layout ``layout`` (1, 2 or 4:
    :meth:`GraphPlan.new_records`, ``maxk_topk_cbsr_records``), the table
    :meth:`GraphPlan.forward_records` gathers as it is. The plain tables are still written and
    returned; with ``return_values=False`` (records only) the ``[N, k]`` value table is
    neither allocated nor written and ``None`` stands in its place in the result.
    ``dropout=(p, seed)`` or ``(p, seed, row_offset)``: feature dropout fused into the top-k
    (``maxk_topk_cbsr_dropout``): the emitted values, in tables, records and statistics alike,
    are ``keep ? x / (1 - p) : +0.0`` with the counter-based mask of include/maxk_hip.h keyed on
    ``(seed, row_offset + row, feature)``; selectors and counts are those of the undropped
    input. ``seed`` is any int, taken modulo 2^64. ``None`` or ``p == 0`` is today's path.
    ``dense``: an f32 ``[N, D]`` tensor on the input's device, contiguous or row-strided (unit
    column stride, row stride >= D), that receives the dense masked row with the same launch
    (``maxk_topk_cbsr_dense``): ``dense[r, f]`` is the value the table holds for the filled
    slot that selected ``f`` (dropped and scaled under ``dropout``), ``+0.0`` for every other
    feature. It must not overlap ``input``. The return value is unchanged; with ``dense`` given,
    ``return_values=False`` needs no ``records``.
    """
    _need(input.is_cuda, "input must be a CUDA tensor")
    _need(input.is_contiguous(), "input must be contiguous")
    _need(input.dim() == 2, "Input must be 2D tensor")
    n, d = input.shape
    _need(1 <= k <= d, "k must be between 1 and input dimension")
    _need(d <= 256, "input dimension must be <= 256 (u8 selectors)")
    _need(input.dtype == torch.float32, "input must be float32")
    _need(mode in TOPK_MODES, f"mode must be one of {sorted(TOPK_MODES)}")
    _need(return_values or records is not None or dense is not None,
          "return_values=False needs records")
    dstride = 0
    if dense is not None:
        _need(isinstance(dense, torch.Tensor) and dense.is_cuda and dense.device == input.device,
              "dense must be a CUDA tensor on the input's device")
        _need(dense.dtype == torch.float32, "dense must be float32")
        dstride = _table(dense, "dense", torch.float32, n, d)
    if out is None:
        sp_data = (torch.empty((n, k), dtype=torch.float32, device=input.device)
                   if return_values else None)
        sp_index = torch.empty((n, k), dtype=torch.uint8, device=input.device)
        ds = is_ = k
    else:
        sp_data, sp_index = out
        _need(sp_data.device == input.device and sp_index.device == input.device,
              "out must be on the input's device")
        ds = _table(sp_data, "out[0]", torch.float32, n, k)
        is_ = _table(sp_index, "out[1]", torch.uint8, n, k)
    if not return_values:
        sp_data = None  # neither written nor returned
    values = _p(sp_data)
    count = torch.empty(n, dtype=torch.int32, device=input.device) if return_count else None
    scratch, sbytes = None, 0
    if stats is not None:
        _need(stats.is_cuda and stats.device == input.device and stats.is_contiguous() and
              stats.dtype == torch.int32 and stats.numel() == 2,
              "stats must be a contiguous int32 CUDA tensor of 2 elements on the input's device")
        sbytes = int(lib.maxk_topk_stats_scratch_bytes(n))
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=input.device)
    drop = _dropout_arg(dropout)
    buf, layout, rb = None, 0, 0
    if records is not None:
        buf, layout = records
        rb = _records(buf, layout, n, k, "records")
        _need(buf.device == input.device, "records must be on the input's device")
    with _device(input.device):
        if dense is not None:
            p, seed, row_offset = drop if drop is not None else (0.0, 0, 0)
            check(lib.maxk_topk_cbsr_dense(_p(input), _p(dense), dstride, _p(buf), rb, int(layout),
                                           values, ds, _p(sp_index), is_, _p(count), _p(stats),
                                           _p(scratch), sbytes, n, d, k, TOPK_MODES[mode], p,
                                           seed, row_offset, _stream()), "maxk_forward")
        elif drop is not None:
            check(lib.maxk_topk_cbsr_dropout(_p(input), _p(buf), rb, int(layout), values, ds,
                                             _p(sp_index), is_, _p(count), _p(stats), _p(scratch),
                                             sbytes, n, d, k, TOPK_MODES[mode], drop[0], drop[1],
                                             drop[2], _stream()), "maxk_forward")
        elif records is not None:
            check(lib.maxk_topk_cbsr_records(_p(input), _p(buf), rb, int(layout), values, ds,
                                             _p(sp_index), is_, _p(count), _p(stats), _p(scratch),
                                             sbytes, n, d, k, TOPK_MODES[mode], _stream()),
                  "maxk_forward")
        else:
            check(lib.maxk_topk_cbsr_ex(_p(input), values, ds, _p(sp_index), is_, _p(count),
                                        _p(stats), _p(scratch), sbytes, n, d, k,
                                        TOPK_MODES[mode], _stream()), "maxk_forward")
    res = (sp_data, sp_index) if return_index else (sp_data,)
    if return_count:
        res = res + (count,)
    return res if len(res) > 1 else res[0]


def maxk_backward(grad_output: Optional[torch.Tensor], indices: torch.Tensor,
                  dim_origin: Optional[int] = None, dropout=None,
                  grad_dense: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense gradient of MaxK from the ``[N, k]`` CBSR gradient.

    Reference (maxk_backward_cuda SO@0x21410): ``g = zeros(N, max(indices)+1)``;
    ``g[i, indices[i, j]] = grad_output[i, j]`` for j ascending. Checks (bindings.cpp:34-36):
    grad_output CUDA/contiguous/2-D, indices CUDA/contiguous. Here one device kernel does
    the scatter; pass ``dim_origin`` for a stable ``[N, dim_origin]`` shape (without it the
    reference's data-dependent width ``max(indices)+1`` is kept, which costs a host sync).
    ``dropout`` as for :func:`maxk_forward` (``maxk_scatter_backward_dropout``): each loaded
    value becomes ``keep(row, selector) ? g / (1 - p) : +0.0``, the backward of the top-k
    called with the same tuple.
    ``grad_dense``: the f32 ``[N, dim_origin]`` gradient of the dense masked row
    (:func:`maxk_forward` ``dense=``; rows may be strided), added at the selected features
    before the dropout factor (``maxk_scatter_backward_merge``):
    ``keep ? (grad_dense[r, f] + grad_output[r, j]) / (1 - p) : +0.0``; features no slot selects
    stay 0 whatever ``grad_dense`` holds there. With it ``grad_output`` may be ``None`` (only
    the dense output was used); the shape then comes from ``indices`` and ``dim_origin``.
    """
    _need(indices.is_cuda, "indices must be a CUDA tensor")
    if grad_output is None:
        _need(grad_dense is not None, "grad_output=None needs grad_dense")
        _need(indices.dim() == 2, "indices must be 2D tensor")
        device = indices.device
    else:
        _need(grad_output.is_cuda, "grad_output must be a CUDA tensor")
        _need(grad_output.is_contiguous(), "grad_output must be contiguous")
        _need(grad_output.dim() == 2, "grad_output must be 2D tensor")
        _need(indices.shape == grad_output.shape, "indices must have the shape of grad_output")
        _need(grad_output.dtype == torch.float32, "grad_output must be float32")
        device = grad_output.device
    n, k = indices.shape
    # u8 selectors may be row-strided (the interleaved records of maxk_aggregate); other
    # integer dtypes are converted (contiguous)
    strided_u8 = (indices.dtype == torch.uint8 and indices.dim() == 2 and
                  (n <= 1 or indices.stride(1) == 1) and (n <= 1 or indices.stride(0) >= k))
    _need(indices.is_contiguous() or strided_u8, "indices must be contiguous")
    if indices.dtype != torch.uint8:
        _need(not indices.dtype.is_floating_point, "indices must be an integer tensor")
        indices = indices.to(torch.uint8)
    istride = indices.stride(0) if n > 1 else k
    if dim_origin is None:
        dim_origin = int(indices.max().item()) + 1 if indices.numel() else 1
    _need(1 <= k <= dim_origin <= 256, "k must be between 1 and input dimension")
    grad_in = torch.empty((n, dim_origin), dtype=torch.float32, device=device)
    drop = _dropout_arg(dropout)
    with _device(device):
        if grad_dense is not None:
            _need(isinstance(grad_dense, torch.Tensor) and grad_dense.is_cuda and
                  grad_dense.device == device, "grad_dense must be a CUDA tensor on the same device")
            gstride = _table(grad_dense, "grad_dense", torch.float32, n, dim_origin)
            p, seed, row_offset = drop if drop is not None else (0.0, 0, 0)
            check(lib.maxk_scatter_backward_merge(_p(grad_output), _p(indices), istride,
                                                  _p(grad_dense), gstride, _p(grad_in), n,
                                                  dim_origin, k, p, seed, row_offset, _stream()),
                  "maxk_backward")
        elif drop is not None:
            check(lib.maxk_scatter_backward_dropout(_p(grad_output), _p(indices), istride,
                                                    _p(grad_in), n, dim_origin, k, drop[0],
                                                    drop[1], drop[2], _stream()),
                  "maxk_backward")
        else:
            check(lib.maxk_scatter_backward_tables(_p(grad_output), _p(indices), istride,
                                                   _p(grad_in), n, dim_origin, k, _stream()),
                  "maxk_backward")
    return grad_in


# -------------------------------------------------------------------------------------
# graph plans (cached partition metadata)
# -------------------------------------------------------------------------------------
class GraphPlan:
    """Owns one ``maxk_plan`` (device partition metadata for a CSR graph, k and D).

    The plan is built with ``external_workspace``: its per-call scratch (packed CBSR records,
    selector words, the two-pass E x k products) is taken from torch's caching allocator on
    the launch stream for every call, so no plan pins that memory and one plan can serve
    several streams at once. The only mutation after creation, a value refresh, is ordered
    after every earlier use on other streams (an event recorded on each of them at refresh
    time, i.e. after everything they queued) and every later use after it; calls record
    nothing (a per-call event cost ~10 us of host time on small graphs).
    """

    def __init__(self, ptr, idx, val, num_nodes, num_edges, dim_origin, dim_k,
                 num_cols: Optional[int] = None, options: Optional[dict] = None,
                 col_order: Optional[torch.Tensor] = None):
        """``options``: ``maxk_plan_options`` fields by name (``col_order`` also by name:
        'identity', 'scattered'; ``bwd_algo``: 'column_blocks', 'two_pass'); ``col_order``: an
        int32 device permutation of the columns (position -> column) for the backward's
        column blocks, which selects ``col_order='given'``. Building allocates and synchronises
        the stream, so it is refused while a graph is being captured."""
        _refuse_capture("GraphPlan (building a plan)",
                        "build the plan before capture (call once eagerly)")
        self.handle = ctypes.c_void_p(0)
        self.device = ptr.device
        self._refs = (ptr, idx, val)  # keep the graph's storage alive while cached
        self.val_version = _version(val)
        self.num_rows = int(num_nodes)
        self.num_cols = int(num_nodes if num_cols is None else num_cols)
        self.num_edges = int(num_edges)
        self.dim_origin = int(dim_origin)
        self.dim_k = int(dim_k)
        opts = PlanOptions()
        opts.external_workspace = 1
        for key, value in (options or {}).items():
            if key in ("fwd_accumulator", "bwd_accumulator") and isinstance(value, str):
                value = ACC_KINDS[value]
            if key == "col_order" and isinstance(value, str):
                value = COL_ORDERS[value]
            if key == "bwd_algo" and isinstance(value, str):
                value = BWD_ALGOS[value]
            setattr(opts, key, int(value))
        if col_order is not None:
            _check_tensor(col_order, "col_order", torch.int32)
            _need(col_order.numel() == self.num_cols, "col_order must have num_cols entries")
            opts.col_order = COL_ORDERS["given"]
        with torch.cuda.device(ptr.device):
            check(lib.maxk_plan_create_sized(_p(ptr), _p(idx), _p(val), self.num_rows,
                                             self.num_cols, self.num_edges, self.dim_origin,
                                             self.dim_k, ctypes.byref(opts),
                                             ctypes.sizeof(opts), _p(col_order), _stream(),
                                             ctypes.byref(self.handle)), "maxk_plan_create")
        fb, bb = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib.maxk_plan_workspace_bytes(self.handle, ctypes.byref(fb), ctypes.byref(bb)),
              "maxk_plan_workspace_bytes")
        self.external = bool(opts.external_workspace)
        self.fwd_ws_bytes, self.bwd_ws_bytes = int(fb.value), int(bb.value)
        self._uses = {}        # stream id -> a stream the plan was used on
        self._refresh = None   # (stream, event) of the latest value refresh
        self._lock = threading.Lock()

    # -- stream ordering ------------------------------------------------------------------
    def _begin(self, stream):
        with self._lock:
            if self._refresh is not None and self._refresh[0] != stream:
                stream.wait_event(self._refresh[1])

    def _end(self, stream):
        sid = stream.cuda_stream
        if sid not in self._uses:
            with self._lock:
                self._uses[sid] = stream

    def _workspace(self, nbytes):
        if not self.external or nbytes == 0:
            return None, 0
        try:
            return torch.empty(nbytes, dtype=torch.uint8, device=self.device), nbytes
        except torch.OutOfMemoryError:
            # the two-pass backward's product workspace is the large one (one row chunk of
            # E x k x 4 bytes, <= 16 GiB by default, kBwdTwoPassWorkspaceCap): give the
            # allocator its cached blocks back once, then say which knob bounds it
            torch.cuda.empty_cache()
            try:
                return torch.empty(nbytes, dtype=torch.uint8, device=self.device), nbytes
            except torch.OutOfMemoryError as exc:
                raise torch.OutOfMemoryError(
                    f"maxk_kernels: per-call workspace of {nbytes} bytes does not fit; a plan "
                    f"built with options={{'bwd_tp_chunks': P}} (more row chunks) or "
                    f"{{'bwd_algo': 1}} (column blocks) needs less") from exc

    @staticmethod
    def _stats_arg(stats):
        """``stats`` of :meth:`forward` as (tensor, pairs, stride in 32-bit words)."""
        if isinstance(stats, tuple):
            st, n_st, stride = stats
            _need(st.is_cuda and st.element_size() == 4 and
                  (n_st - 1) * stride + 2 <= st.numel(), "stats does not hold n pairs")
            return st, n_st, stride
        if stats is not None:
            _need(stats.is_cuda and stats.is_contiguous() and stats.dtype == torch.int32 and
                  stats.dim() == 2 and stats.shape[1] == 2 and stats.shape[0] >= 1,
                  "stats must be a contiguous int32 [n, 2] CUDA tensor")
            return stats, stats.shape[0], 2
        return None, 0, 2

    def forward(self, sp_data, sp_index, out=None, accumulate: bool = False,
                stats=None) -> torch.Tensor:
        """SpGEMM with this plan: sp tables [num_cols, k] (rows may be strided, e.g. the
        interleaved records of :mod:`maxk_kernels.dist`, gathered in place) -> out [num_rows, D];
        ``accumulate=True`` adds into the given ``out`` instead of overwriting it. ``stats``:
        fixed-point statistics covering the table instead of a pass over it, either an int32
        [n, 2] tensor of :func:`cbsr_stats` pairs or ``(tensor, n, stride)`` with pair i at
        32-bit word i * stride of the tensor's storage (the multi-GPU path keeps one pair
        per rank in a spare row of the gathered table). Without ``stats`` the call scans
        every row of the tables, so each row must be CBSR data: a ShardedAggregation's
        gathered table is not (its spare rows hold those pairs), pass its ``stats``."""
        ptr, idx, val = self._refs
        if out is None:
            if accumulate:
                raise RuntimeError("accumulate=True needs an out tensor")
            out = torch.empty((self.num_rows, self.dim_origin), dtype=torch.float32,
                              device=sp_data.device)
        stream = torch.cuda.current_stream(self.device)
        self._begin(stream)
        ws, wsb = self._workspace(self.fwd_ws_bytes)
        st, n_st, stride = self._stats_arg(stats)
        ds = _table(sp_data, "sp_data", torch.float32, self.num_cols, self.dim_k)
        is_ = _table(sp_index, "sp_index", torch.uint8, self.num_cols, self.dim_k)
        check(lib.maxk_spgemm_forward_tables(self.handle, _p(ptr), _p(idx), _p(val), _p(sp_data),
                                             ds, _p(sp_index), is_, _p(out), self.num_rows,
                                             self.num_edges, self.dim_k, self.dim_origin,
                                             int(accumulate), _p(st), n_st, stride, _p(ws), wsb,
                                             ctypes.c_void_p(stream.cuda_stream)),
              "spgemm_forward")
        self._end(stream)
        return out

    def forward_records(self, records, layout, out=None, accumulate: bool = False,
                        stats=None) -> torch.Tensor:
        """SpGEMM from chunk records the caller holds in this plan's layout (``records`` u8
        [num_cols, record_bytes] and ``layout`` as :meth:`new_records` returns them, written by
        :func:`maxk_forward` ``records=``) -> out [num_rows, D]: the forward kernel alone (and
        the zeroing of split rows), no pack, no statistics pass, no workspace
        (``maxk_spgemm_forward_records``). ``stats`` as for :meth:`forward`; required when
        ``info()['fwd_fixed']`` is 1."""
        ptr, idx, val = self._refs
        rb = _records(records, layout, self.num_cols, self.dim_k, "records")
        if out is None:
            if accumulate:
                raise RuntimeError("accumulate=True needs an out tensor")
            out = torch.empty((self.num_rows, self.dim_origin), dtype=torch.float32,
                              device=records.device)
        stream = torch.cuda.current_stream(self.device)
        self._begin(stream)
        st, n_st, stride = self._stats_arg(stats)
        check(lib.maxk_spgemm_forward_records(self.handle, _p(ptr), _p(idx), _p(val),
                                              _p(records), rb, int(layout), _p(out),
                                              self.num_rows, self.num_edges, self.dim_k,
                                              self.dim_origin, int(accumulate), _p(st), n_st,
                                              stride, ctypes.c_void_p(stream.cuda_stream)),
              "spgemm_forward_records")
        self._end(stream)
        return out

    def backward(self, grad_out, sp_index, grad_sp=None) -> torch.Tensor:
        """SSpMM with this plan: grad_out [num_rows, D] -> grad_sp [num_cols, k]."""
        ptr, idx, val = self._refs
        if grad_sp is None:
            grad_sp = torch.empty((self.num_cols, self.dim_k), dtype=torch.float32,
                                  device=grad_out.device)
        stream = torch.cuda.current_stream(self.device)
        self._begin(stream)
        ws, wsb = self._workspace(self.bwd_ws_bytes)
        is_ = _table(sp_index, "sp_index", torch.uint8, self.num_cols, self.dim_k)
        check(lib.maxk_sspmm_backward_tables(self.handle, _p(ptr), _p(idx), _p(val),
                                             _p(grad_out), _p(sp_index), is_, _p(grad_sp),
                                             self.num_rows, self.num_edges, self.dim_k,
                                             self.dim_origin, _p(ws), wsb,
                                             ctypes.c_void_p(stream.cuda_stream)),
              "spgemm_backward")
        self._end(stream)
        return grad_sp

    def refresh_values(self, val: torch.Tensor) -> None:
        """Re-snapshot in-place-modified edge values (same tensor, new ``_version``); runs
        after every earlier use of the plan on any stream. It allocates stream-ordered scratch,
        tests the new values for row-constancy where the forward has a 4-byte edge-word form
        (``info()['fwd_rowconst']`` may change; that read-back synchronises the stream)
        and orders itself across streams with events, and a replay would skip its host
        bookkeeping, so it is refused while a graph is being captured (that covers
        ``edge_weight=`` and :func:`get_plan` after an in-place edit of ``val``)."""
        _refuse_capture("GraphPlan.refresh_values (edge_weight=, or edge values edited in place)",
                        "a captured step computes with the edge values of capture time; refresh "
                        "the plan outside the capture and capture again")
        stream = torch.cuda.current_stream(self.device)
        with self._lock:
            for other in self._uses.values():
                if other != stream:  # after everything queued on it so far
                    ev = torch.cuda.Event()
                    ev.record(other)
                    stream.wait_event(ev)
        with torch.cuda.device(self.device):
            check(lib.maxk_plan_refresh_values(self.handle, _p(val),
                                               ctypes.c_void_p(stream.cuda_stream)),
                  "maxk_plan_refresh_values")
        ev = torch.cuda.Event()
        ev.record(stream)
        with self._lock:
            self._refresh = (stream, ev)
            self._uses[stream.cuda_stream] = stream
        self._refs = (self._refs[0], self._refs[1], val)
        self.val_version = _version(val)

    def info(self) -> dict:
        info = PlanInfo()
        check(lib.maxk_plan_get_info_sized(self.handle, ctypes.byref(info), ctypes.sizeof(info)),
              "maxk_plan_get_info")
        d = info.as_dict()
        d["fwd_workspace_bytes"] = self.fwd_ws_bytes
        d["bwd_workspace_bytes"] = self.bwd_ws_bytes
        # 1: 4-byte forward edge words and one value per row (the values of the last build or
        # refresh were row-constant); changes with refresh_values, so read every time
        rc = ctypes.c_int32(0)
        check(lib.maxk_plan_fwd_rowconst(self.handle, ctypes.byref(rc)), "maxk_plan_fwd_rowconst")
        d["fwd_rowconst"] = int(rc.value)
        return d

    @property
    def device_bytes(self) -> int:
        return int(self.info()["device_bytes"])

    def _fwd_layout(self):
        """(fwd_layout, fwd_record_bytes, fwd_fixed) of the plan, read once."""
        layout = getattr(self, "_layout", None)
        if layout is None:
            info = self.info()
            layout = self._layout = (info["fwd_layout"], info["fwd_record_bytes"],
                                     info["fwd_fixed"])
        return layout

    @property
    def fwd_fixed(self) -> bool:
        """Whether the forward runs fixed point, i.e. consumes the statistics pair."""
        return bool(self._fwd_layout()[2])

    def new_records(self):
        """``(records, layout)`` for :func:`maxk_forward` ``records=`` and
        :meth:`forward_records`: an uninitialised u8 [num_cols, fwd_record_bytes] buffer and the
        plan's ``fwd_layout`` when that is 1 (packed), 2 (lane chunks) or 4 (pair chunks);
        ``None`` when the forward gathers the two plain tables (layouts 0 and 3)."""
        layout, rec_bytes, _ = self._fwd_layout()
        if layout not in (1, 2, 4):
            return None
        return (torch.empty((self.num_cols, rec_bytes), dtype=torch.uint8, device=self.device),
                layout)

    def new_cbsr(self):
        """Uninitialised ``(sp_data, sp_index)`` [num_cols, k] tables in the layout this plan's
        forward gathers (``fwd_layout``): strided views of one buffer of packed records
        (``fwd_record_bytes`` per column, values then selectors) when the forward reads packed
        records, so a top-k written there (:func:`maxk_forward` ``out=``) needs no per-call
        pack; two plain tables otherwise."""
        layout = self._fwd_layout()
        n, k = self.num_cols, self.dim_k
        if layout[0] == 1 and n > 0:
            rec = torch.empty((n, layout[1]), dtype=torch.uint8, device=self.device)
            return rec[:, :4 * k].view(torch.float32), rec[:, 4 * k:5 * k]
        return (torch.empty((n, k), dtype=torch.float32, device=self.device),
                torch.empty((n, k), dtype=torch.uint8, device=self.device))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and lib is not None:
            lib.maxk_plan_destroy(h)
            self.handle = ctypes.c_void_p(0)


# Plans are cached per (graph structure, edge-value tensor, k, D): two value sets on one
# structure (SAGE 'mean' and GCN 'both' weights, say) get two plans instead of refreshing
# one plan back and forth. The cache is bounded by the device memory the plans hold
# (MAXK_PLAN_CACHE_BYTES, default a quarter of the device's HBM: ~72 GB on MI355X, twenty
# Reddit-sized plans) and by a count.
_PLAN_CACHE: "collections.OrderedDict[tuple, GraphPlan]" = collections.OrderedDict()
_PLAN_CACHE_SIZE = 32
_PLAN_CACHE_BYTES: Optional[int] = (int(os.environ["MAXK_PLAN_CACHE_BYTES"])
                                    if "MAXK_PLAN_CACHE_BYTES" in os.environ else None)
_PLAN_LOCK = threading.Lock()


def _cache_budget(device) -> int:
    if _PLAN_CACHE_BYTES is not None:
        return _PLAN_CACHE_BYTES
    return torch.cuda.get_device_properties(device).total_memory // 4


def _values_stale(plan, val) -> bool:
    """Whether ``plan``'s value snapshot is of another tensor than ``val``, or of ``val`` before
    an in-place edit: a ``refresh_values(val)`` is due."""
    return plan._refs[2] is not val or plan.val_version != _version(val)


def get_plan(ptr, idx, val, num_nodes, num_edges, dim_origin, dim_k) -> GraphPlan:
    """Cached plan for (graph storage, structure version, value tensor, k, D); in-place
    edits of ``val`` (a new ``val._version``) refresh the plan's value snapshot.

    The key is ``(device, ptr/idx data_ptr, ptr/idx _version, val data_ptr, N, E, D, k)``, so an
    edit is seen only through torch's version counter. Edits that bypass it are unsupported:
    after ``idx.data.copy_(...)`` (``.data`` has a version counter of its own), or a write
    through a raw pointer, the cached plan of the old structure or values keeps being served.
    Call :func:`clear_plan_cache` after such an edit, or edit the tensor itself
    (``idx.copy_(...)``, ``val.mul_(...)``)."""
    key = (ptr.device.index, ptr.data_ptr(), idx.data_ptr(), _version(ptr), _version(idx),
           val.data_ptr(), int(num_nodes), int(num_edges), int(dim_origin), int(dim_k))
    with _PLAN_LOCK:
        plan = _PLAN_CACHE.get(key)
        if plan is not None:
            _PLAN_CACHE.move_to_end(key)
            if _values_stale(plan, val):
                plan.refresh_values(val)
            return plan
        plan = GraphPlan(ptr, idx, val, int(num_nodes), int(num_edges), int(dim_origin),
                         int(dim_k))
        _PLAN_CACHE[key] = plan
        budget = _cache_budget(ptr.device)
        total = sum(p.device_bytes for p in _PLAN_CACHE.values())
        while len(_PLAN_CACHE) > 1 and (len(_PLAN_CACHE) > _PLAN_CACHE_SIZE or total > budget):
            _, old = _PLAN_CACHE.popitem(last=False)
            total -= old.device_bytes
        return plan


def cached_plan_bytes() -> int:
    with _PLAN_LOCK:
        return sum(p.device_bytes for p in _PLAN_CACHE.values())


def clear_plan_cache() -> None:
    with _PLAN_LOCK:
        _PLAN_CACHE.clear()


def _check_graph(ptr, idx, val, num_nodes, num_edges):
    _check_tensor(ptr, "ptr", torch.int32)
    _check_tensor(idx, "idx", torch.int32)
    _check_tensor(val, "val", torch.float32)
    _need(ptr.dim() == 1 and ptr.numel() == num_nodes + 1, "ptr must have num_nodes+1 entries")
    _need(idx.numel() == num_edges and val.numel() == num_edges,
          "idx and val must have num_edges entries")


# -------------------------------------------------------------------------------------
# SpGEMM forward / SSpMM backward
# -------------------------------------------------------------------------------------
def _resolve_plan(plan, ptr, idx, val, num_nodes, num_edges, dim_k, dim_origin, tables):
    """The argument checks of :func:`spgemm_forward` and :func:`spgemm_backward`, and the plan
    they run on: the caller's, or the cached one. ``tables``: ``(tensor, name, dtype, shape,
    message for another shape)`` per table argument. The graph is checked unless it is the
    plan's own, whose tensors were checked when it was built."""
    if plan is None or plan._refs[0] is not ptr or plan._refs[1] is not idx or plan._refs[2] is not val:
        _check_graph(ptr, idx, val, num_nodes, num_edges)
    for t, name, dtype, _, _ in tables:
        _check_tensor(t, name, dtype)
    for t, _, _, shape, message in tables:
        _need(t.shape == shape, message)
    _need(1 <= dim_k <= dim_origin <= 256, "k must be between 1 and input dimension")
    if plan is None:
        plan = get_plan(ptr, idx, val, num_nodes, num_edges, dim_origin, dim_k)
    _need(plan.num_rows == num_nodes and plan.num_edges == num_edges and
          plan.dim_k == dim_k and plan.dim_origin == dim_origin,
          "plan was built for a different graph / k / D")
    return plan


def spgemm_forward(ptr, idx, val, sp_data, sp_index, num_nodes: int, num_edges: int,
                   dim_k: int, dim_origin: int, plan: Optional[GraphPlan] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-wise-product SpGEMM over CBSR features.

    Reference ``spgemm_forward(ptr, idx, val, sp_data, sp_index, num_nodes, num_edges,
    dim_k, dim_origin) -> (out[num_nodes, dim_origin], sp_index)`` (spgemm_forward_cuda
    SO@0x221a0; checks bindings.cpp:45-54): ``out[r] = sum_nz val[nz] *
    densify(sp_data[idx[nz]], sp_index[idx[nz]])``.
    """
    shape, message = (num_nodes, dim_k), "sp_data and sp_index must be [num_nodes, dim_k]"
    plan = _resolve_plan(plan, ptr, idx, val, num_nodes, num_edges, dim_k, dim_origin,
                         ((sp_data, "sp_data", torch.float32, shape, message),
                          (sp_index, "sp_index", torch.uint8, shape, message)))
    with _device(sp_data.device):
        out = plan.forward(sp_data, sp_index)
    return out, sp_index


def spgemm_backward(ptr, idx, val, grad_output, sp_index, num_nodes: int, num_edges: int,
                    dim_k: int, dim_origin: int, plan: Optional[GraphPlan] = None
                    ) -> torch.Tensor:
    """Outer-product SSpMM: ``grad_sp[c, l] = sum_{(r,c)} val * grad_output[r, sp_index[c, l]]``.

    Reference ``spgemm_backward(ptr, idx, val, grad_output, sp_index, num_nodes,
    num_edges, dim_k, dim_origin) -> [num_nodes, dim_k]`` (spgemm_backward_cuda
    SO@0x22490; checks bindings.cpp:65-71).
    """
    plan = _resolve_plan(plan, ptr, idx, val, num_nodes, num_edges, dim_k, dim_origin,
                         ((grad_output, "grad_output", torch.float32, (num_nodes, dim_origin),
                           "grad_output must be [num_nodes, dim_origin]"),
                          (sp_index, "sp_index", torch.uint8, (num_nodes, dim_k),
                           "sp_index must be [num_nodes, dim_k]")))
    with _device(grad_output.device):
        grad_sp = plan.backward(grad_output, sp_index)
    return grad_sp


def spgemm_edge_grad(ptr, idx, grad_output, sp_data, sp_index, num_nodes: int, num_edges: int,
                     dim_k: int, dim_origin: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of :func:`spgemm_forward` with respect to ``val``: the sampled dense-dense
    product ``grad_val[e] = sum_l sp_data[c, l] * grad_output[r, sp_index[c, l]]`` for edge
    ``e = (r, c)``, f32 ``[num_edges]`` in CSR edge order (``maxk_sddmm_edge_grad``; the
    summation order is pinned in include/maxk_hip.h). It depends on neither ``val`` nor a
    plan. ``grad_output`` is ``[num_nodes, dim_origin]`` (rows may be strided); the tables have
    one row per source column (their row count is the number of columns, so a rectangular
    shard works) and may be strided, e.g. interleaved records. ``out``: a contiguous f32
    ``[num_edges]`` tensor to write into."""
    _check_tensor(ptr, "ptr", torch.int32)
    _check_tensor(idx, "idx", torch.int32)
    _need(ptr.dim() == 1 and ptr.numel() == num_nodes + 1, "ptr must have num_nodes+1 entries")
    _need(idx.numel() == num_edges, "idx must have num_edges entries")
    _need(1 <= dim_k <= dim_origin <= 256, "k must be between 1 and input dimension")
    _need(isinstance(sp_data, torch.Tensor) and sp_data.dim() == 2,
          "sp_data must be [num_cols, dim_k]")
    num_cols = sp_data.shape[0]
    gs = _table(grad_output, "grad_output", torch.float32, num_nodes, dim_origin)
    ds = _table(sp_data, "sp_data", torch.float32, num_cols, dim_k)
    is_ = _table(sp_index, "sp_index", torch.uint8, num_cols, dim_k)
    dev = ptr.device
    _need(idx.device == dev and grad_output.device == dev and sp_data.device == dev and
          sp_index.device == dev, "all tensors must be on the same device")
    if out is None:
        out = torch.empty(num_edges, dtype=torch.float32, device=dev)
    else:
        _check_tensor(out, "out", torch.float32)
        _need(out.dim() == 1 and out.numel() == num_edges and out.device == dev,
              "out must be [num_edges] on the graph's device")
    with _device(dev):
        check(lib.maxk_sddmm_edge_grad(_p(ptr), _p(idx), _p(grad_output), gs, _p(sp_data), ds,
                                       _p(sp_index), is_, _p(out), num_nodes, num_cols,
                                       num_edges, dim_origin, dim_k, _stream()),
              "spgemm_edge_grad")
    return out


def _edge_softmax_args(ptr, tensors, names, out):
    """The checks shared by :func:`edge_softmax` and :func:`edge_softmax_backward`: ``ptr`` int32
    ``[num_rows + 1]``, every tensor of ``tensors`` contiguous f32 ``[num_edges]`` on ``ptr``'s
    device. Returns ``(num_rows, num_edges, out)``."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    num_edges = None
    for t, name in zip(tensors, names):
        _check_tensor(t, name, torch.float32)
        _need(t.dim() == 1, f"{name} must be [num_edges]")
        num_edges = t.numel() if num_edges is None else num_edges
        _need(t.numel() == num_edges, f"{name} must have num_edges entries")
        _need(t.device == dev, "all tensors must be on the same device")
    if out is None:
        out = torch.empty(num_edges, dtype=torch.float32, device=dev)
    else:
        _check_tensor(out, "out", torch.float32)
        _need(out.dim() == 1 and out.numel() == num_edges and out.device == dev,
              "out must be [num_edges] on the graph's device")
    return ptr.numel() - 1, num_edges, out


def edge_softmax(ptr, logits, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Softmax of the per-edge ``logits`` (f32 ``[num_edges]``, CSR edge order) over each
    destination row's in-edges ``[ptr[r], ptr[r + 1])``: DGL's ``edge_softmax`` on the in-edge
    CSR (``maxk_edge_softmax_forward``; semantics and accuracy in include/maxk_hip.h, "Edge
    softmax"). ``ptr[-1] == num_edges`` is a precondition (it is not read on the host).
    ``out``: a contiguous f32 ``[num_edges]`` tensor to write into."""
    n, e, out = _edge_softmax_args(ptr, (logits,), ("logits",), out)
    with _device(ptr.device):
        check(lib.maxk_edge_softmax_forward(_p(ptr), _p(logits), _p(out), n, e, _stream()),
              "edge_softmax")
    return out


def edge_softmax_backward(ptr, y, grad_y, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of :func:`edge_softmax` with respect to the logits, from its output ``y`` and
    the gradient ``grad_y`` of that output: ``y * (grad_y - sum_row(y * grad_y))``
    (``maxk_edge_softmax_backward``)."""
    n, e, out = _edge_softmax_args(ptr, (y, grad_y), ("y", "grad_y"), out)
    with _device(ptr.device):
        check(lib.maxk_edge_softmax_backward(_p(ptr), _p(y), _p(grad_y), _p(out), n, e,
                                             _stream()), "edge_softmax_backward")
    return out


def _int32_list(fn, *args) -> Tuple[int, ...]:
    """The list behind an export ``fn(*args, out, capacity) -> count``: asked for its count, then
    read in full."""
    count = fn(*args, None, 0)
    buf = (ctypes.c_int32 * count)()
    fn(*args, ctypes.cast(buf, ctypes.c_void_p), count)
    return tuple(int(v) for v in buf)


def edge_softmax_row_limits() -> Tuple[int, ...]:
    """The row lengths at which the edge-softmax kernels switch regime, ascending
    (``maxk_edge_softmax_row_limits``): a row of exactly a limit's length runs in the regime
    below it."""
    return _int32_list(lib.maxk_edge_softmax_row_limits)


def _vector(t, name: str, dtype: torch.dtype, size, size_name: str, dev) -> None:
    """A contiguous 1-D ``dtype`` tensor of ``size`` entries (``None``: any) on ``dev``."""
    _check_tensor(t, name, dtype)
    _need(t.dim() == 1 and (size is None or t.numel() == size), f"{name} must be [{size_name}]")
    _need(t.device == dev, "all tensors must be on the same device")


def _gat_attention_args(ptr, idx, el, er):
    """The checks shared by :func:`gat_attention` and :func:`gat_attention_backward`: ``ptr``
    int32 ``[num_rows + 1]``, ``idx`` int32 ``[num_edges]``, ``el`` f32 ``[num_cols]``, ``er`` f32
    ``[num_rows]`` on ``ptr``'s device. Returns ``(num_rows, num_cols, num_edges)``."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    _vector(el, "el", torch.float32, None, "num_cols", dev)
    _vector(er, "er", torch.float32, ptr.numel() - 1, "num_rows", dev)
    return ptr.numel() - 1, el.numel(), idx.numel()


def _out_vector(out, name: str, size: int, size_name: str, dev) -> torch.Tensor:
    if out is None:
        return torch.empty(size, dtype=torch.float32, device=dev)
    _check_tensor(out, name, torch.float32)
    _need(out.dim() == 1 and out.numel() == size and out.device == dev,
          f"{name} must be [{size_name}] on the graph's device")
    return out


def gat_attention(ptr, idx, el, er, negative_slope: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention weights of single-head GAT from the two node score vectors, one kernel: the
    :func:`edge_softmax` of ``leaky_relu(el[idx] + er[row], negative_slope)`` over each row's
    in-edges, bit for bit, with no ``[num_edges]`` intermediate (``maxk_gat_attention_forward``;
    include/maxk_hip.h, "GAT attention"). ``el`` is f32 ``[num_cols]`` (the source side), ``er``
    f32 ``[num_rows]``; ``idx`` lies in ``[0, num_cols)`` and ``ptr[-1] == num_edges`` (neither is
    read on the host). ``out``: a contiguous f32 ``[num_edges]`` tensor to write into."""
    n, c, e = _gat_attention_args(ptr, idx, el, er)
    out = _out_vector(out, "out", e, "num_edges", ptr.device)
    with _device(ptr.device):
        check(lib.maxk_gat_attention_forward(_p(ptr), _p(idx), _p(el), _p(er),
                                             float(negative_slope), _p(out), n, c, e, _stream()),
              "gat_attention")
    return out


def gat_attention_backward(ptr, idx, el, er, negative_slope: float, alpha, grad_alpha,
                           out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(grad_edge [num_edges], grad_er [num_rows])`` of :func:`gat_attention` from its output
    ``alpha`` and that output's gradient: ``grad_edge`` is the gradient with respect to the sum
    ``el[idx] + er[row]`` (the softmax backward through the leaky-relu branch of the recomputed
    score), ``grad_er`` its sum over each row in a fixed order
    (``maxk_gat_attention_backward``). ``grad_el`` is :func:`edge_colsum` of ``grad_edge``.
    ``out=(grad_edge, grad_er)``: contiguous f32 tensors to write into."""
    n, c, e = _gat_attention_args(ptr, idx, el, er)
    dev = ptr.device
    _vector(alpha, "alpha", torch.float32, e, "num_edges", dev)
    _vector(grad_alpha, "grad_alpha", torch.float32, e, "num_edges", dev)
    grad_edge, grad_er = out if out is not None else (None, None)
    grad_edge = _out_vector(grad_edge, "out[0]", e, "num_edges", dev)
    grad_er = _out_vector(grad_er, "out[1]", n, "num_rows", dev)
    with _device(dev):
        check(lib.maxk_gat_attention_backward(_p(ptr), _p(idx), _p(el), _p(er),
                                              float(negative_slope), _p(alpha), _p(grad_alpha),
                                              _p(grad_edge), _p(grad_er), n, c, e, _stream()),
              "gat_attention_backward")
    return grad_edge, grad_er


def edge_colsum(ptr_t, order, values, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum of the per-edge ``values`` (f32 ``[num_edges]``, CSR edge order) over each source
    column, f32 ``[num_cols]``, in a fixed order and without atomics (``maxk_edge_colsum``):
    ``out[c] = sum_j values[order[j]]`` for ``j`` in ``[ptr_t[c], ptr_t[c + 1])``, with ``ptr_t``
    int32 ``[num_cols + 1]`` and ``order`` int32 ``[num_edges]`` the transposed structure of the
    graph (``CSRGraph.transposed_structure()[0]`` and ``CSRGraph.transposed_order()``)."""
    _check_ptr(ptr_t, "ptr_t", "num_cols")
    dev = ptr_t.device
    _vector(order, "order", torch.int32, None, "num_edges", dev)
    _vector(values, "values", torch.float32, order.numel(), "num_edges", dev)
    c = ptr_t.numel() - 1
    out = _out_vector(out, "out", c, "num_cols", dev)
    with _device(dev):
        check(lib.maxk_edge_colsum(_p(ptr_t), _p(order), _p(values), _p(out), c, order.numel(),
                                   _stream()), "edge_colsum")
    return out


# -------------------------------------------------------------------------------------
# Multi-head attention and aggregation (include/maxk_hip.h, "GAT attention, heads" and
# "Multi-head aggregation"); every per-head array is head-major
# -------------------------------------------------------------------------------------
def _matrix(t, name: str, rows, cols, shape_name: str, dev) -> None:
    """A contiguous f32 ``[rows, cols]`` tensor (``None``: any extent) on ``dev``."""
    _check_tensor(t, name, torch.float32)
    _need(t.dim() == 2 and (rows is None or t.shape[0] == rows) and
          (cols is None or t.shape[1] == cols), f"{name} must be [{shape_name}]")
    _need(t.device == dev, "all tensors must be on the same device")


def _out_matrix(out, name: str, rows: int, cols: int, shape_name: str, dev) -> torch.Tensor:
    if out is None:
        return torch.empty((rows, cols), dtype=torch.float32, device=dev)
    _matrix(out, name, rows, cols, shape_name, dev)
    return out


def _gat_heads_args(ptr, idx, el, er):
    """``ptr`` int32 ``[num_rows + 1]``, ``idx`` int32 ``[num_edges]``, ``el`` f32 ``[H,
    num_cols]``, ``er`` f32 ``[H, num_rows]``. Returns ``(H, num_rows, num_cols, num_edges)``."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    _matrix(el, "el", None, None, "num_heads, num_cols", dev)
    _need(el.shape[0] >= 1, "el must have at least one head")
    _matrix(er, "er", el.shape[0], ptr.numel() - 1, "num_heads, num_rows", dev)
    return el.shape[0], ptr.numel() - 1, el.shape[1], idx.numel()


def gat_attention_heads(ptr, idx, el, er, negative_slope: float,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`gat_attention` for ``H`` heads in one launch: ``el`` f32 ``[H, num_cols]``, ``er``
    f32 ``[H, num_rows]``, the result ``alpha`` f32 ``[H, num_edges]``; row ``h`` is the
    single-head call on row ``h`` bit for bit (``maxk_gat_attention_forward_heads``)."""
    h, n, c, e = _gat_heads_args(ptr, idx, el, er)
    out = _out_matrix(out, "out", h, e, "num_heads, num_edges", ptr.device)
    with _device(ptr.device):
        check(lib.maxk_gat_attention_forward_heads(_p(ptr), _p(idx), _p(el), _p(er),
                                                   float(negative_slope), _p(out), h, n, c, e,
                                                   _stream()), "gat_attention_heads")
    return out


def gat_attention_backward_heads(ptr, idx, el, er, negative_slope: float, alpha, grad_alpha,
                                 out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(grad_edge [H, num_edges], grad_er [H, num_rows])`` of :func:`gat_attention_heads`
    (``maxk_gat_attention_backward_heads``); ``grad_el`` is :func:`edge_colsum_heads` of
    ``grad_edge``."""
    h, n, c, e = _gat_heads_args(ptr, idx, el, er)
    dev = ptr.device
    _matrix(alpha, "alpha", h, e, "num_heads, num_edges", dev)
    _matrix(grad_alpha, "grad_alpha", h, e, "num_heads, num_edges", dev)
    grad_edge, grad_er = out if out is not None else (None, None)
    grad_edge = _out_matrix(grad_edge, "out[0]", h, e, "num_heads, num_edges", dev)
    grad_er = _out_matrix(grad_er, "out[1]", h, n, "num_heads, num_rows", dev)
    with _device(dev):
        check(lib.maxk_gat_attention_backward_heads(_p(ptr), _p(idx), _p(el), _p(er),
                                                    float(negative_slope), _p(alpha),
                                                    _p(grad_alpha), _p(grad_edge), _p(grad_er), h,
                                                    n, c, e, _stream()),
              "gat_attention_backward_heads")
    return grad_edge, grad_er


def edge_colsum_heads(ptr_t, order, values, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`edge_colsum` of ``values`` f32 ``[H, num_edges]`` per head: f32 ``[H, num_cols]``
    (``maxk_edge_colsum_heads``)."""
    _check_ptr(ptr_t, "ptr_t", "num_cols")
    dev = ptr_t.device
    _vector(order, "order", torch.int32, None, "num_edges", dev)
    _matrix(values, "values", None, order.numel(), "num_heads, num_edges", dev)
    _need(values.shape[0] >= 1, "values must have at least one head")
    h, c = values.shape[0], ptr_t.numel() - 1
    out = _out_matrix(out, "out", h, c, "num_heads, num_cols", dev)
    with _device(dev):
        check(lib.maxk_edge_colsum_heads(_p(ptr_t), _p(order), _p(values), _p(out), h, c,
                                         order.numel(), _stream()), "edge_colsum_heads")
    return out


def _heads_tables(sp_data, sp_index, dev):
    """The plain CBSR tables ``[num_cols, k]`` (rows may be strided): ``(num_cols, k, ds, is)``."""
    _need(isinstance(sp_data, torch.Tensor) and sp_data.dim() == 2,
          "sp_data must be [num_cols, dim_k]")
    num_cols, k = sp_data.shape
    ds = _table(sp_data, "sp_data", torch.float32, num_cols, k)
    is_ = _table(sp_index, "sp_index", torch.uint8, num_cols, k)
    _need(sp_data.device == dev and sp_index.device == dev,
          "all tensors must be on the same device")
    return num_cols, k, ds, is_


_NO_ALPHA = object()


def _aggregate_backward_args(ptr_t, idx_t, order, grad_out, alpha=_NO_ALPHA):
    """The transposed structure and the ``grad_out`` table of an aggregation's backward, with the
    head-major ``alpha [H, num_edges]`` of the multi-head one checked between them:
    ``(device, num_edges, num_rows, dim_origin, grad_stride)``."""
    _check_ptr(ptr_t, "ptr_t", "num_cols")
    dev = ptr_t.device
    _vector(order, "order", torch.int32, None, "num_edges", dev)
    e = order.numel()
    _vector(idx_t, "idx_t", torch.int32, e, "num_edges", dev)
    if alpha is not _NO_ALPHA:
        _matrix(alpha, "alpha", None, e, "num_heads, num_edges", dev)
    _need(isinstance(grad_out, torch.Tensor) and grad_out.dim() == 2,
          "grad_out must be [num_rows, dim_origin]")
    n, d = grad_out.shape
    gs = _table(grad_out, "grad_out", torch.float32, n, d)
    _need(grad_out.device == dev, "all tensors must be on the same device")
    return dev, e, n, d, gs


def heads_aggregate(ptr, idx, alpha, sp_data, sp_index, dim_origin: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Multi-head weighted aggregation of CBSR features, f32 ``[num_rows, dim_origin]``:
    ``out[r, s] = sum_e alpha[s // F, e] * X[idx[e], s]`` over row ``r``'s edges, with ``alpha``
    f32 ``[H, num_edges]`` head-major, ``F = dim_origin // H`` and ``X`` the densified tables
    (``maxk_heads_aggregate_forward``; contract in include/maxk_hip.h, "Multi-head
    aggregation"). No plan is built or used."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    e, n = idx.numel(), ptr.numel() - 1
    _matrix(alpha, "alpha", None, e, "num_heads, num_edges", dev)
    h = alpha.shape[0]
    _need(1 <= h and int(dim_origin) % max(h, 1) == 0,
          "the number of heads (alpha.shape[0]) must divide dim_origin")
    num_cols, k, ds, is_ = _heads_tables(sp_data, sp_index, dev)
    _need(1 <= k <= dim_origin <= 256, "k must be between 1 and input dimension")
    out = _out_matrix(out, "out", n, int(dim_origin), "num_rows, dim_origin", dev)
    with _device(dev):
        check(lib.maxk_heads_aggregate_forward(_p(ptr), _p(idx), _p(alpha), _p(sp_data), ds,
                                               _p(sp_index), is_, _p(out), h, n, num_cols, e,
                                               int(dim_origin), k, _stream()), "heads_aggregate")
    return out


def heads_aggregate_backward(ptr_t, idx_t, order, alpha, grad_out, sp_data, sp_index,
                             need_sp: bool = True, need_alpha: bool = True):
    """``(grad_sp [num_cols, k] or None, grad_alpha [H, num_edges] or None)`` of
    :func:`heads_aggregate` from one gather of ``grad_out`` (f32 ``[num_rows, dim_origin]``, rows
    may be strided) over the transposed structure ``(ptr_t, idx_t, order)``, all int32
    (``maxk_heads_aggregate_backward``). A half that is not needed is not computed; nothing is
    launched when neither is."""
    dev, e, n, d, gs = _aggregate_backward_args(ptr_t, idx_t, order, grad_out, alpha)
    h = alpha.shape[0]
    _need(1 <= h and d % max(h, 1) == 0,
          "the number of heads (alpha.shape[0]) must divide dim_origin")
    num_cols, k, ds, is_ = _heads_tables(sp_data, sp_index, dev)
    _need(num_cols == ptr_t.numel() - 1, "sp_data must have num_cols rows")
    _need(1 <= k <= d <= 256, "k must be between 1 and input dimension")
    grad_sp = torch.empty((num_cols, k), dtype=torch.float32, device=dev) if need_sp else None
    grad_alpha = torch.empty((h, e), dtype=torch.float32, device=dev) if need_alpha else None
    if need_sp or need_alpha:
        with _device(dev):
            check(lib.maxk_heads_aggregate_backward(_p(ptr_t), _p(idx_t), _p(order), _p(alpha),
                                                    _p(grad_out), gs, _p(sp_data), ds,
                                                    _p(sp_index), is_, _p(grad_sp),
                                                    _p(grad_alpha), h, n, num_cols, e, d, k,
                                                    _stream()), "heads_aggregate_backward")
    return grad_sp, grad_alpha


def heads_row_limits() -> Tuple[int, ...]:
    """``(row_short, row_medium, col_short, col_medium)``: the row lengths at which the
    multi-head forward and the column lengths at which its backward switch regime
    (``maxk_heads_row_limits``); exactly a limit's length runs in the regime below it."""
    return _int32_list(lib.maxk_heads_row_limits)


# -------------------------------------------------------------------------------------
# Max aggregation (include/maxk_hip.h, "Max aggregation")
# -------------------------------------------------------------------------------------
MAX_ROW_EDGES = 1 << 24  # the forward's precondition: every row is shorter than this


def max_aggregate_forward(ptr, idx, sp_data, sp_index, dim_origin: int, with_arg: bool = True):
    """``(out f32, arg_edge int32 or None, arg_slot u8 or None)``, each ``[num_rows,
    dim_origin]``: the element-wise maximum of the densified CBSR rows of each row's in-edges,
    unselected features as implicit zeros, and the winner's CSR edge and slot (``-1``, ``0`` for
    the implicit zero). ``with_arg=False`` writes ``out`` alone, with the same bits
    (``maxk_max_aggregate_forward``). Rows of 2^24 edges or more are not supported and not
    checked here (:func:`maxk_kernels.max_aggregate` checks its graph once)."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    e, n = idx.numel(), ptr.numel() - 1
    num_cols, k, ds, is_ = _heads_tables(sp_data, sp_index, dev)
    d = int(dim_origin)
    _need(1 <= k <= d <= 256, "k must be between 1 and input dimension")
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    arg_edge = torch.empty((n, d), dtype=torch.int32, device=dev) if with_arg else None
    arg_slot = torch.empty((n, d), dtype=torch.uint8, device=dev) if with_arg else None
    with _device(dev):
        check(lib.maxk_max_aggregate_forward(_p(ptr), _p(idx), _p(sp_data), ds, _p(sp_index), is_,
                                             _p(out), _p(arg_edge), _p(arg_slot), n, num_cols, e,
                                             d, k, _stream()), "max_aggregate_forward")
    return out, arg_edge, arg_slot


def max_aggregate_backward(ptr_t, idx_t, order, grad_out, arg_edge, arg_slot,
                           sp_index) -> torch.Tensor:
    """``grad_sp [num_cols, k]`` of :func:`max_aggregate_forward`: each ``grad_out`` element
    (f32 ``[num_rows, dim_origin]``, rows may be strided) goes to the slot that ``arg_edge`` /
    ``arg_slot`` name, summed per slot over the transposed structure ``(ptr_t, idx_t, order)``,
    all int32 (``maxk_max_aggregate_backward``)."""
    dev, e, n, d, gs = _aggregate_backward_args(ptr_t, idx_t, order, grad_out)
    for t, name, dtype in ((arg_edge, "arg_edge", torch.int32), (arg_slot, "arg_slot", torch.uint8)):
        _check_tensor(t, name, dtype)
        _need(tuple(t.shape) == (n, d) and t.device == dev,
              f"{name} must be [num_rows, dim_origin] on the same device")
    _need(isinstance(sp_index, torch.Tensor) and sp_index.dim() == 2,
          "sp_index must be [num_cols, dim_k]")
    num_cols, k = sp_index.shape
    is_ = _table(sp_index, "sp_index", torch.uint8, num_cols, k)
    _need(sp_index.device == dev, "all tensors must be on the same device")
    _need(num_cols == ptr_t.numel() - 1, "sp_index must have num_cols rows")
    _need(1 <= k <= d <= 256, "k must be between 1 and input dimension")
    grad_sp = torch.empty((num_cols, k), dtype=torch.float32, device=dev)
    with _device(dev):
        check(lib.maxk_max_aggregate_backward(_p(ptr_t), _p(idx_t), _p(order), _p(grad_out), gs,
                                              _p(arg_edge), _p(arg_slot), _p(sp_index), is_,
                                              _p(grad_sp), n, num_cols, e, d, k, _stream()),
              "max_aggregate_backward")
    return grad_sp


def max_row_limits() -> Tuple[int, ...]:
    """``(row_short, row_medium, col_short, col_medium)`` of the max aggregation's forward and
    backward (``maxk_max_row_limits``); exactly a limit's length runs in the regime below it."""
    return _int32_list(lib.maxk_max_row_limits)


# -------------------------------------------------------------------------------------
# Neighbour sampling (include/maxk_hip.h, "Neighbour sampling")
# -------------------------------------------------------------------------------------
def _scratch(scratch, nbytes: int, dev) -> torch.Tensor:
    if scratch is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _check_tensor(scratch, "scratch", torch.uint8)
    _need(scratch.dim() == 1 and scratch.numel() >= nbytes and scratch.device == dev,
          f"scratch must be a u8 tensor of at least {nbytes} bytes on the same device")
    return scratch


def sample_capacity(num_edges: int, num_seeds: int, fanout: int) -> int:
    """Entries of ``out_col`` / ``out_eid`` that hold every result of distinct seeds:
    ``min(num_edges, num_seeds * fanout)``, ``num_edges`` for ``fanout < 0``."""
    return int(num_edges) if fanout < 0 else min(int(num_edges), int(num_seeds) * int(fanout))


def sample_neighbors(ptr, idx, seeds, fanout: int, seed: int, out=None, scratch=None):
    """``(out_ptr int32 [S + 1], out_col int32 [capacity], out_eid int32 [capacity])``: at most
    ``fanout`` in-edges of each seed row, chosen by the rank rule of the header, in ascending
    edge number (``maxk_sample_neighbors``). The buffers come back whole: entries at and past
    ``out_ptr[S]`` are not written, and nothing is read back here. ``out``: the three buffers,
    pre-allocated (``capacity = out[1].numel()``; default :func:`sample_capacity`); ``scratch``: a
    u8 buffer of :func:`sample_scratch_bytes` bytes. With both given the call allocates nothing
    and can be captured into a graph."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    _vector(seeds, "seeds", torch.int32, None, "num_seeds", dev)
    n, e, s, fanout = ptr.numel() - 1, idx.numel(), seeds.numel(), int(fanout)
    _need(fanout != 0, "fanout must be positive, or negative for every neighbour")
    if out is None:
        cap = sample_capacity(e, s, fanout)
        out = (torch.empty(s + 1, dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.int32, device=dev))
    out_ptr, out_col, out_eid = out
    _vector(out_ptr, "out_ptr", torch.int32, s + 1, "num_seeds + 1", dev)
    _vector(out_col, "out_col", torch.int32, None, "capacity", dev)
    _vector(out_eid, "out_eid", torch.int32, out_col.numel(), "capacity", dev)
    nbytes = sample_scratch_bytes(s)
    scratch = _scratch(scratch, nbytes, dev)
    with _device(dev):
        check(lib.maxk_sample_neighbors(_p(ptr), _p(idx), _p(seeds), _p(out_ptr), _p(out_col),
                                        _p(out_eid), out_col.numel(), _p(scratch),
                                        scratch.numel(), n, e, s, fanout,
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
              "sample_neighbors")
    return out_ptr, out_col, out_eid


def sample_scratch_bytes(num_seeds: int) -> int:
    return int(lib.maxk_sample_scratch_bytes(int(num_seeds)))


def block_compact_scratch_bytes(num_cols: int) -> int:
    return int(lib.maxk_block_compact_scratch_bytes(int(num_cols)))


def block_compact(seeds, cols, num_cols: int, out=None, scratch=None):
    """``(src_ids int32 [capacity], local_col int32 [num_edges], counts int32 [2])``: the seeds,
    then every other column of ``cols`` once in ascending order; ``cols`` mapped to positions in
    ``src_ids``; ``counts = {num_src, distinct_seeds}`` on the device (``maxk_block_compact``).
    ``src_ids`` comes back whole (``capacity = num_seeds + min(num_edges, num_cols)`` by default)
    and nothing is read back here. ``out`` / ``scratch`` (:func:`block_compact_scratch_bytes`
    bytes, u8) as for :func:`sample_neighbors`."""
    _check_tensor(seeds, "seeds", torch.int32)
    dev = seeds.device
    _vector(seeds, "seeds", torch.int32, None, "num_seeds", dev)
    _vector(cols, "cols", torch.int32, None, "num_edges", dev)
    s, m, num_cols = seeds.numel(), cols.numel(), int(num_cols)
    _need(num_cols >= 0, "num_cols must not be negative")
    if out is None:
        out = (torch.empty(s + min(m, num_cols), dtype=torch.int32, device=dev),
               torch.empty(m, dtype=torch.int32, device=dev),
               torch.empty(2, dtype=torch.int32, device=dev))
    src_ids, local_col, counts = out
    _vector(src_ids, "src_ids", torch.int32, None, "capacity", dev)
    _vector(local_col, "local_col", torch.int32, m, "num_edges", dev)
    _vector(counts, "counts", torch.int32, 2, "2", dev)
    scratch = _scratch(scratch, block_compact_scratch_bytes(num_cols), dev)
    with _device(dev):
        check(lib.maxk_block_compact(_p(seeds), _p(cols), _p(src_ids), src_ids.numel(),
                                     _p(local_col), _p(counts), _p(scratch), scratch.numel(), s,
                                     m, num_cols, _stream()), "block_compact")
    return src_ids, local_col, counts


def sample_row_limits() -> Tuple[int, ...]:
    """``(short, medium)``: the row lengths at which the sampler switches regime
    (``maxk_sample_row_limits``); exactly a limit's length runs in the regime below it."""
    return _int32_list(lib.maxk_sample_row_limits)


# -------------------------------------------------------------------------------------
# Induced subgraphs (include/maxk_hip.h, "Induced subgraphs")
# -------------------------------------------------------------------------------------
def induced_subgraph_scratch_bytes(num_nodes: int, num_sel: int) -> int:
    return int(lib.maxk_induced_subgraph_scratch_bytes(int(num_nodes), int(num_sel)))


def _subgraph_args(ptr, idx, nodes):
    _check_ptr(ptr, "ptr", "num_nodes")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    _vector(nodes, "nodes", torch.int32, None, "num_sel", dev)
    return ptr.numel() - 1, idx.numel(), nodes.numel(), dev


def induced_subgraph_count(ptr, idx, nodes, out=None, scratch=None):
    """``(out_ptr int32 [S + 1], counts int32 [3])`` of ``A[nodes][:, nodes]``: the exclusive
    scan of the kept edges per position of ``nodes``, and ``{M, distinct nodes, entries out of
    range}`` on the device (``maxk_induced_subgraph_count``). Nothing is read back here. ``out``:
    the two buffers, pre-allocated; ``scratch``: a u8 buffer of
    :func:`induced_subgraph_scratch_bytes` bytes. With both given the call allocates nothing and
    can be captured into a graph."""
    n, e, s, dev = _subgraph_args(ptr, idx, nodes)
    if out is None:
        out = (torch.empty(s + 1, dtype=torch.int32, device=dev),
               torch.empty(3, dtype=torch.int32, device=dev))
    out_ptr, counts = out
    _vector(out_ptr, "out_ptr", torch.int32, s + 1, "num_sel + 1", dev)
    _vector(counts, "counts", torch.int32, 3, "3", dev)
    scratch = _scratch(scratch, induced_subgraph_scratch_bytes(n, s), dev)
    with _device(dev):
        check(lib.maxk_induced_subgraph_count(_p(ptr), _p(idx), _p(nodes), _p(out_ptr),
                                              _p(counts), _p(scratch), scratch.numel(), n, e, s,
                                              _stream()), "induced_subgraph_count")
    return out_ptr, counts


def induced_subgraph_fill(ptr, idx, nodes, out_ptr, capacity: Optional[int] = None, out=None,
                          scratch=None):
    """``(out_col int32 [capacity], out_eid int32 [capacity])``: the local column and the edge
    number in the parent of every kept edge, behind the ``out_ptr`` of
    :func:`induced_subgraph_count` on the same inputs (``maxk_induced_subgraph_fill``). Entries at
    and past ``out_ptr[S]`` are not written, and nothing is read back here. ``out``: the two
    buffers, pre-allocated (``capacity = out[0].numel()``); ``scratch`` as for the count."""
    n, e, s, dev = _subgraph_args(ptr, idx, nodes)
    _vector(out_ptr, "out_ptr", torch.int32, s + 1, "num_sel + 1", dev)
    if out is None:
        _need(capacity is not None and int(capacity) >= 0, "capacity or out must be given")
        out = (torch.empty(int(capacity), dtype=torch.int32, device=dev),
               torch.empty(int(capacity), dtype=torch.int32, device=dev))
    out_col, out_eid = out
    _vector(out_col, "out_col", torch.int32, None, "capacity", dev)
    _vector(out_eid, "out_eid", torch.int32, out_col.numel(), "capacity", dev)
    scratch = _scratch(scratch, induced_subgraph_scratch_bytes(n, s), dev)
    with _device(dev):
        check(lib.maxk_induced_subgraph_fill(_p(ptr), _p(idx), _p(nodes), _p(out_ptr),
                                             _p(out_col), _p(out_eid), out_col.numel(),
                                             _p(scratch), scratch.numel(), n, e, s, _stream()),
              "induced_subgraph_fill")
    return out_col, out_eid


def subgraph_row_limits() -> Tuple[int, ...]:
    """``(short, medium)``: the row lengths at which the extraction switches regime
    (``maxk_subgraph_row_limits``); exactly a limit's length runs in the regime below it."""
    return _int32_list(lib.maxk_subgraph_row_limits)


# -------------------------------------------------------------------------------------
# CSR transposition (include/maxk_hip.h, "CSR transposition")
# -------------------------------------------------------------------------------------
def csr_transpose_scratch_bytes(num_rows: int, num_cols: int, num_edges: int) -> int:
    return int(lib.maxk_csr_transpose_scratch_bytes(int(num_rows), int(num_cols),
                                                    int(num_edges)))


def transpose_digit_bits(num_cols: int) -> Tuple[int, ...]:
    """The digit widths, lowest digit first, of the radix passes :func:`csr_transpose` runs for
    ``num_cols`` columns (``maxk_transpose_digit_bits``)."""
    return _int32_list(lib.maxk_transpose_digit_bits, int(num_cols))


def csr_transpose(ptr, idx, val=None, num_cols: Optional[int] = None, out=None, scratch=None):
    """``(ptr_t int32 [num_cols + 1], idx_t int32 [E], order int32 [E][, val_t f32 [E]])``: A^T of
    the CSR graph ``(ptr, idx)`` of ``num_cols`` columns (default: square), by the rule of the
    header (``maxk_csr_transpose``): edge ``j`` of A^T is edge ``order[j]`` of A, the edges of a
    column in ascending edge number, ``idx_t`` their rows, ``val_t = val[order]`` bit for bit
    (returned when ``val`` is given). ``out``: the three or four buffers, pre-allocated;
    ``scratch``: a u8 buffer of :func:`csr_transpose_scratch_bytes` bytes. With both given the
    call allocates nothing and can be captured into a graph."""
    _check_ptr(ptr, "ptr", "num_rows")
    dev = ptr.device
    _vector(idx, "idx", torch.int32, None, "num_edges", dev)
    n, e = ptr.numel() - 1, idx.numel()
    nc = n if num_cols is None else int(num_cols)
    _need(nc >= 0, "num_cols must not be negative")
    if val is not None:
        _vector(val, "val", torch.float32, e, "num_edges", dev)
    if out is None:
        out = (torch.empty(nc + 1, dtype=torch.int32, device=dev),
               torch.empty(e, dtype=torch.int32, device=dev),
               torch.empty(e, dtype=torch.int32, device=dev))
        if val is not None:
            out += (torch.empty(e, dtype=torch.float32, device=dev),)
    _need(len(out) == (3 if val is None else 4),
          "out must hold ptr_t, idx_t, order, and val_t exactly when val is given")
    _vector(out[0], "ptr_t", torch.int32, nc + 1, "num_cols + 1", dev)
    _vector(out[1], "idx_t", torch.int32, e, "num_edges", dev)
    _vector(out[2], "order", torch.int32, e, "num_edges", dev)
    if val is not None:
        _vector(out[3], "val_t", torch.float32, e, "num_edges", dev)
    scratch = _scratch(scratch, csr_transpose_scratch_bytes(n, nc, e), dev)
    with _device(dev):
        check(lib.maxk_csr_transpose(_p(ptr), _p(idx), _p(val), _p(out[0]), _p(out[1]),
                                     _p(out[2]), _p(out[3] if val is not None else None),
                                     _p(scratch), scratch.numel(), n, nc, e, _stream()),
              "csr_transpose")
    return tuple(out)


def plan_col_order(plan: GraphPlan) -> torch.Tensor:
    """The plan's column order: int32 [num_cols], position -> column of the backward's column
    blocks (the identity for plans without one)."""
    out = torch.empty(plan.num_cols, dtype=torch.int32, device=plan.device)
    with torch.cuda.device(plan.device):
        check(lib.maxk_plan_get_col_order(plan.handle, _p(out), _stream()), "plan_col_order")
    return out


def cbsr_stats(sp_data: torch.Tensor, sp_index: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fixed-point statistics of a CBSR table (``maxk_cbsr_stats``): int32 [1, 2] (written
    into ``out`` when given), the pair :meth:`GraphPlan.forward` takes as ``stats``."""
    _need(sp_data.dim() == 2 and sp_index.shape == sp_data.shape,
          "sp_data and sp_index must be [N, k]")
    n, k = sp_data.shape
    ds = _table(sp_data, "sp_data", torch.float32, n, k)
    is_ = _table(sp_index, "sp_index", torch.uint8, n, k)
    if out is None:
        out = torch.empty((1, 2), dtype=torch.int32, device=sp_data.device)
    _need(out.is_cuda and out.is_contiguous() and out.dtype == torch.int32 and out.numel() == 2,
          "out must be a contiguous int32 CUDA tensor of 2 elements")
    with torch.cuda.device(sp_data.device):
        check(lib.maxk_cbsr_stats_tables(_p(sp_data), ds, _p(sp_index), is_, n, k, _p(out),
                                         _stream()), "cbsr_stats")
    return out


def dense_spmm(ptr, idx, val, x) -> torch.Tensor:
    """Dense CSR SpMM comparator (DGL ``update_all(copy_u, sum)`` with edge weights). The
    kernel takes float4 rows: other widths run on a copy padded to a multiple of 4 features
    (zeros; DGL's SAGEConv/GraphConv/GINConv accept any hidden size)."""
    _check_tensor(x, "x", torch.float32)
    _check_graph(ptr, idx, val, x.shape[0], idx.numel())
    _need(x.dim() == 2, "x must be 2D")
    d = x.shape[1]
    d4 = (d + 3) // 4 * 4
    xin = x if d4 == d else torch.nn.functional.pad(x, (0, d4 - d)).contiguous()
    y = torch.empty_like(xin)
    with torch.cuda.device(x.device):
        check(lib.maxk_dense_spmm_csr(_p(ptr), _p(idx), _p(val), _p(xin), _p(y), x.shape[0],
                                      d4, _stream()), "dense_spmm")
    return y if d4 == d else y[:, :d].contiguous()
