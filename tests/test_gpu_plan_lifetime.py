"""GPU: what a plan holds, for how long, and which plan a call gets.

The 18 plan arrays are owning device buffers (``DeviceBuf`` members of ``maxk_plan``, freed by
its destructor), the build's temporaries are ``DeviceBuf`` locals of the build's stages, and
``device_bytes`` is summed by the one function that allocates a plan array (``plan_alloc``, or
``plan_adopt`` for a scratch buffer promoted into the plan); ``device_bytes`` is the only
input of the plan cache's byte budget, and autograd contexts keep plans alive past eviction.
None of that changes an output, so these tests read the device's free memory instead.

How memory is read. ``level()`` is ``torch.cuda.mem_get_info()[0]`` after a synchronise plus
``torch.cuda.memory_reserved()``: a drop of the level is memory taken outside torch's
allocator. Per-call workspaces and outputs come from torch's and cancel out. The scratch of
``maxk_plan_refresh_values`` and of the fixed-point bounds comes from the runtime's
stream-ordered pool (``hipMallocAsync``), which is not corrected for: a warm-up absorbs a
constant reserve, and a scratch block that is never freed shows as lost free memory. A reading
is taken until it repeats: the free-memory figure can lag a ``hipFree`` that has returned by
one reading (the reading taken immediately after a short one is exact; a leak does not come
back). Two more things are measured, not assumed:

* the ``hipMalloc`` granule G of this runtime (fixture ``granule``): raw allocations of sizes
  just past 1 B, 4 KiB, 1, 2, 5 and 64 MiB; G is the smallest power of two above every
  (drop - size), and every drop must then be at most ceil(size / G) * G and come back on free.
  Each non-null array of a plan rounds up by less than G, so a comparison of held memory with
  ``device_bytes`` has the slack (non-null arrays) x G; the accounting graphs have 4 E > 2 x 18 G.
* whether anything else moves the card's free memory (``measured``): two readings around an
  idle wait of about the measurement's duration (the timed warm-up's, then the measurement's
  own) come before each measurement; when they differ by more than G the measurement is
  repeated, three times in all, then the test fails with the drifts.

Which case is meant to make which plan array non-null (CASES[...]["sets"]; the accounting test
derives each plan's non-null set from its info and options, checks it contains these, and the
report at the end checks that the union is all 18):

  default_k16            fwd_tasks fwd_perm fwd_cv fwd_fix fwd_rowptr fwd_phase_off
                         bwd_tasks bwd_perm bwd_rec
  k8_lane_chunks         (forward layout 2, no fixed point: no fwd_fix / fwd_rowptr)
  k8_fixed               fwd_fix fwd_rowptr
  k32_packed             (forward layout 1)
  k16_float              (fwd_fixed off at k = 16)
  heavy_row              zero_rows
  slabs                  bwd_combine
  slabs_owned_ws         bwd_combine bwd_sel fwd_rec
  two_pass_1             bwd_erec bwd_colptr
  two_pass_7_owned_ws    bwd_erec bwd_colptr bwd_colptr2 bwd_tbuf
  scattered, given       bwd_corder
  owned_ws               fwd_rec
  rect                   (N != num_cols)
  no_edges, no_nodes     (E = 0: forward arrays only; N = 0: nothing)
  tall                   fwd_tasks fwd_fix fwd_rowptr fwd_phase_off, each above the slack
                         (4 x 10^7 edgeless rows)
  wide_two_pass_7        bwd_colptr bwd_colptr2 above the slack (2 x 10^7 columns)
  wide_scattered         bwd_corder above the slack

  split_everything       zero_rows bwd_tasks bwd_combine above the slack (6 x 10^6 rows of two
                         edges, every row split, every edge a backward piece of its own)

``tall``, the two ``wide`` cases and ``split_everything`` exist because on the common graph the
arrays sized by N, by num_cols or by a task count are smaller than the slack: there a missed
``device_bytes +=`` for them would pass. No kernel of the compute path runs on them.

What a leak test can see. This runtime serves allocations below a granule as fragments of
shared 2 MiB blocks (measured: the edgeless plan's two arrays move the free memory by nothing),
so a leaked array shows only once the leaks fill blocks: ten cycles see a leak of about 0.4 MiB
per cycle or more. The cycles therefore run on the accounting graphs (E-sized arrays of 72 MiB,
N-sized ones of 0.75 MiB) and on ``tall`` (task-sized arrays of 10 MiB and more). ``zero_rows``,
``bwd_tasks`` and ``bwd_combine`` are kilobytes on every graph a forward or backward is
affordable on, below what the cycles resolve; their frees are checked by the accounting test
of ``split_everything``, where they are 24 MiB and more and destroy has to give back what the
plan held.

The out-of-range ``idx`` refusal is included: sort_bwd_blocks reads the key kernel's ``bad``
flag right after the block sort, and every kernel before that point uses a column id as a value
(sort keys, edge words) or clamped (``bwd_key_kernel``), never as an index.
"""
import ctypes
import gc
import time

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import _lib, ops
from oracle import oracle

pytestmark = pytest.mark.gpu

lib = _lib.lib
P = ctypes.c_void_p
D = 64                       # dim_origin of every plan here
CYCLES = 10
ARRAYS = ("fwd_tasks", "fwd_rec", "fwd_perm", "fwd_cv", "fwd_fix", "fwd_rowptr", "fwd_phase_off",
          "zero_rows", "bwd_tasks", "bwd_perm", "bwd_rec", "bwd_sel", "bwd_colptr", "bwd_erec",
          "bwd_tbuf", "bwd_combine", "bwd_colptr2", "bwd_corder")
COMMON = {"fwd_tasks", "fwd_perm", "fwd_cv", "fwd_phase_off", "bwd_perm"}
BLOCKS = COMMON | {"bwd_tasks", "bwd_rec"}

# name -> k, graph, options (external_workspace 1 unless given, as GraphPlan builds its plans),
# the arrays the case is meant to set, the forward layout it is meant to take
CASES = {
    "default_k16": dict(k=16, sets=BLOCKS | {"fwd_fix", "fwd_rowptr"}, layout=4),
    "k8_lane_chunks": dict(k=8, sets=BLOCKS, unset={"fwd_fix", "fwd_rowptr"}, layout=2),
    "k8_fixed": dict(k=8, opts=dict(fwd_fixed=1), sets=BLOCKS | {"fwd_fix", "fwd_rowptr"},
                     layout=2),
    "k32_packed": dict(k=32, opts=dict(fwd_two_tables=2), sets=BLOCKS | {"fwd_fix"}, layout=1),
    "k16_float": dict(k=16, opts=dict(fwd_fixed=2), sets=BLOCKS, unset={"fwd_fix", "fwd_rowptr"},
                      layout=4),
    "heavy_row": dict(k=16, graph="heavy", sets=BLOCKS | {"zero_rows"}),
    "slabs": dict(k=16, opts=dict(bwd_algo=1, bwd_piece_edges="E/400"),
                  sets=BLOCKS | {"bwd_combine"}, unset={"bwd_sel", "fwd_rec"}),
    "slabs_owned_ws": dict(k=16, opts=dict(bwd_algo=1, bwd_piece_edges="E/400",
                                           external_workspace=0),
                           sets=BLOCKS | {"bwd_combine", "bwd_sel", "fwd_rec"}),
    "two_pass_1": dict(k=16, opts=dict(bwd_algo=3, bwd_tp_chunks=1),
                       sets=COMMON | {"bwd_erec", "bwd_colptr"},
                       unset={"bwd_colptr2", "bwd_tbuf", "bwd_rec", "bwd_tasks"}),
    "two_pass_7_owned_ws": dict(k=16, opts=dict(bwd_algo=3, bwd_tp_chunks=7, external_workspace=0),
                                sets=COMMON | {"bwd_erec", "bwd_colptr", "bwd_colptr2", "bwd_tbuf",
                                               "fwd_rec"}),
    "scattered": dict(k=16, opts=dict(bwd_algo=1, col_order=2), sets=BLOCKS | {"bwd_corder"}),
    "given": dict(k=16, opts=dict(bwd_algo=1), given=True, sets=BLOCKS | {"bwd_corder"}),
    "owned_ws": dict(k=16, opts=dict(external_workspace=0), sets=BLOCKS | {"fwd_rec"}),
    "rect": dict(k=16, graph="rect", sets=BLOCKS),
    "no_edges": dict(k=8, graph="no_edges", sets={"fwd_tasks", "fwd_phase_off"},
                     unset=set(ARRAYS) - {"fwd_tasks", "fwd_phase_off"}),
    "no_nodes": dict(k=8, graph="no_nodes", sets=set(), unset=set(ARRAYS)),
}
# accounting only (no kernels are run on them): arrays sized by N or num_cols above the slack
SHAPE_CASES = {
    "split_everything": dict(k=8, graph="pairs",
                             opts=dict(fwd_task_cap=1, bwd_algo=1, bwd_lds_bytes=56,
                                       bwd_piece_edges=1), warm_up=False,
                             sets=BLOCKS | {"zero_rows", "bwd_combine"},
                             unset={"fwd_fix", "fwd_rowptr", "bwd_sel", "fwd_rec"}),
    "tall": dict(k=16, graph="tall", opts=dict(fwd_fixed=1),
                 sets={"fwd_tasks", "fwd_fix", "fwd_rowptr", "fwd_phase_off"},
                 unset=set(ARRAYS) - {"fwd_tasks", "fwd_fix", "fwd_rowptr", "fwd_phase_off"}),
    "wide_two_pass_7": dict(k=16, graph="wide", opts=dict(bwd_algo=3, bwd_tp_chunks=7),
                            sets=COMMON | {"bwd_erec", "bwd_colptr", "bwd_colptr2"}),
    "wide_scattered": dict(k=16, graph="wide", opts=dict(bwd_algo=1, col_order=2),
                           sets=BLOCKS | {"bwd_corder"}),
}

# what ran, for test_plan_lifetime_report (file order: it runs last)
ROWS = []                    # (case, held, device_bytes, slack, non-null arrays)
COVERED = {}                 # array -> the accounting cases that had it non-null
RAN = {"accounting": set(), "cycles": 0, "refused": 0}
T0 = time.time()


# =========================================================================== reading memory
def level():
    """Free device memory plus what torch's allocator holds: drops by what anyone else takes.
    Read until two readings in a row agree (the figure can lag a hipFree by one reading)."""
    torch.cuda.synchronize()

    def read():
        return torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved()

    prev = read()
    for _ in range(4):
        cur = read()
        if cur == prev:
            break
        prev = cur
    return prev


def mib(b):
    return f"{b / 2 ** 20:.2f} MiB"


def _hip_runtime():
    """The HIP runtime this process already runs on (torch's), for raw hipMalloc / hipFree."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    assert path, "no libamdhip64 is mapped into this process"
    hip = ctypes.CDLL(path)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMalloc.restype = ctypes.c_int
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipFree.restype = ctypes.c_int
    return hip


@pytest.fixture(scope="module")
def granule(gpu):
    torch.empty(1, device=gpu)
    mk.clear_plan_cache()        # plans earlier modules left behind would be freed mid-measurement
    gc.collect()
    hip = _hip_runtime()
    probes = [1, 4097, (1 << 20) + 1, (2 << 20) + 1, (5 << 20) + 1, (64 << 20) + 1]
    rows = []
    for size in probes:
        for _ in range(3):                       # a quiet moment: the same level twice
            a = level()
            if level() == a:
                break
        q = ctypes.c_void_p(0)
        assert hip.hipMalloc(ctypes.byref(q), size) == 0 and q.value
        b = level()
        assert hip.hipFree(q) == 0
        rows.append((size, a - b, level() - b))
    over = max(drop - size for size, drop, _ in rows)
    g = 4096
    while g <= over:
        g *= 2
    print("\nplan lifetime: hipMalloc probes (size, drop of free memory, rise on free): "
          + ", ".join(f"({s}, {d}, {r})" for s, d, r in rows))
    print(f"plan lifetime: measured hipMalloc granule G = {g} bytes ({mib(g)})")
    assert g <= 8 << 20, f"granule {g}: the accounting graphs would need E > {9 * g}"
    for size, drop, back in rows:
        assert drop <= -(-size // g) * g, (size, drop, g)
        assert back == drop, f"hipFree gave back {back} of the {drop} bytes a {size}-byte array took"
    return g


def timed(fn):
    """(seconds ``fn()`` took, its result): the warm-up whose duration seeds ``measured``."""
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def measured(g, fn, wait):
    """``fn()`` (one whole measurement, repeatable) after a quiet check: two levels around an idle
    wait of about its duration (``wait`` seconds, a timed warm-up's, at first; at most 1 s);
    repeated when they differ by more than a granule."""
    drifts = []
    for _ in range(3):
        a = level()
        time.sleep(min(wait, 1.0))
        b = level()
        t0 = time.perf_counter()
        res = fn()
        wait = time.perf_counter() - t0
        if abs(b - a) <= g:
            return res
        drifts.append(b - a)
    pytest.fail(f"the card's free memory never stood still: it moved by {drifts} bytes over idle "
                f"waits (granule {g}); someone else is allocating on this device")


# =========================================================================== graphs
def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def ptr_of(t):
    return P(t.data_ptr()) if t is not None and t.numel() else None


class Graph:
    def __init__(self, ptr, idx, val, n, nc):
        self.ptr, self.idx, self.val, self.n, self.nc = ptr, idx, val, n, nc
        self.e = idx.numel()
        self.val2 = val * 0.5
        self._perm = None
        self._tables = {}

    @property
    def perm(self):
        if self._perm is None:
            gen = torch.Generator(device=self.ptr.device).manual_seed(5)
            self._perm = torch.randperm(self.nc, generator=gen,
                                        device=self.ptr.device).to(torch.int32)
        return self._perm

    def tables(self, k):
        """CBSR tables [nc, k] (ascending distinct selectors) and a gradient [n, D]."""
        if k not in self._tables:
            dev = self.ptr.device
            gen = torch.Generator(device=dev).manual_seed(k)
            sp_data = torch.rand((self.nc, k), generator=gen, device=dev) - 0.5
            sel = (torch.arange(k, device=dev) * (D // k)).to(torch.uint8)
            sp_index = sel.repeat(self.nc, 1).contiguous()
            grad = torch.rand((self.n, D), generator=gen, device=dev) - 0.5
            self._tables[k] = (sp_data, sp_index, grad)
        return self._tables[k]


def build_graphs(dev, n, deg):
    """Uniform-degree graphs built on the device: ``uniform`` (n rows of deg edges, random
    columns), ``heavy`` (row 0 long enough to be split over forward tasks), ``rect`` (columns
    in [0, n / 2)), and the two empty ones."""
    e = n * deg
    gen = torch.Generator(device=dev).manual_seed(11)
    ptr = (torch.arange(n + 1, device=dev, dtype=torch.int64) * deg).to(torch.int32)
    idx = torch.randint(0, n, (e,), generator=gen, device=dev, dtype=torch.int32)
    val = torch.rand(e, generator=gen, device=dev) + 0.5
    heavy = max(3 * 4096, e // 100)
    ptr_h = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                       heavy + (e - heavy) * torch.arange(n, device=dev, dtype=torch.int64)
                       // (n - 1)]).to(torch.int32)
    none_i = torch.empty(0, dtype=torch.int32, device=dev)
    none_f = torch.empty(0, dtype=torch.float32, device=dev)
    return {
        "uniform": Graph(ptr, idx, val, n, n),
        "heavy": Graph(ptr_h, idx, val, n, n),
        "rect": Graph(ptr, idx % (n // 2), val, n, n // 2),
        "no_edges": Graph(torch.zeros(1001, dtype=torch.int32, device=dev), none_i, none_f,
                          1000, 1000),
        "no_nodes": Graph(torch.zeros(1, dtype=torch.int32, device=dev), none_i, none_f, 0, 0),
    }


@pytest.fixture(scope="module")
def big(gpu, granule):
    """The accounting graphs: the smallest E-sized array (4 E bytes) is above twice the largest
    slack, 18 granules."""
    deg = 96
    n = -(-(9 * granule + 1) // deg)
    graphs = build_graphs(gpu, n, deg)
    e = n * deg
    assert 4 * e > 2 * len(ARRAYS) * granule
    gen = torch.Generator(device=gpu).manual_seed(12)
    ncw = max(20_000_000, 10 * granule)           # 4 ncw > 2 x 18 granules too
    assert 4 * ncw > 2 * len(ARRAYS) * granule and ncw <= 1 << 26
    graphs["wide"] = Graph(graphs["uniform"].ptr,
                           torch.randint(0, ncw, (e,), generator=gen, device=gpu,
                                         dtype=torch.int32), graphs["uniform"].val, n, ncw)
    # edgeless rows: 16 + 8 + 8 bytes per 32-row task and 4 per row; the smallest of the four
    # arrays (nt / 4 bytes) is above their slack, 4 granules
    nt = max(40_000_000, 20 * granule)
    assert nt // 4 > 4 * granule and nt < 1 << 31
    graphs["tall"] = Graph(torch.zeros(nt + 1, dtype=torch.int32, device=gpu),
                           torch.empty(0, dtype=torch.int32, device=gpu),
                           torch.empty(0, dtype=torch.float32, device=gpu), nt, 1)
    # two edges per row: with fwd_task_cap = 1 every row is split (zero_rows: 4 B per row), with
    # bwd_piece_edges = 1 every edge is a task (32 B) and, one column per block, every column
    # with two edges or more a split block (16 B); 4 np above the slack of the case's 9 arrays
    npairs = max(6_000_000, 3 * granule)
    graphs["pairs"] = Graph((torch.arange(npairs + 1, device=gpu, dtype=torch.int64) * 2)
                            .to(torch.int32),
                            torch.randint(0, npairs, (2 * npairs,), generator=gen, device=gpu,
                                          dtype=torch.int32),
                            torch.rand(2 * npairs, generator=gen, device=gpu) + 0.5, npairs, npairs)
    print(f"plan lifetime: accounting graphs N = {n}, E = {e} (4 E = {mib(4 * e)}, "
          f"18 G = {mib(18 * granule)}); wide {ncw} columns; tall {nt} rows")
    yield graphs
    graphs.clear()
    torch.cuda.empty_cache()


# =========================================================================== plans
def resolved_options(case, gr):
    opts = {"external_workspace": 1}
    for key, value in case.get("opts", {}).items():
        opts[key] = max(1, gr.e // 400) if value == "E/400" else value
    return opts


def raw_create(gr, k, opts, col_order=None, num_edges=None):
    """maxk_plan_create_sized through the C ABI: (return code, handle)."""
    o = _lib.PlanOptions()
    for key, value in opts.items():
        setattr(o, key, int(value))
    if col_order is not None:
        o.col_order = _lib.COL_ORDERS["given"]
    h = ctypes.c_void_p(0)
    rc = lib.maxk_plan_create_sized(ptr_of(gr.ptr), ptr_of(gr.idx), ptr_of(gr.val), gr.n, gr.nc,
                                    gr.e if num_edges is None else num_edges, D, k,
                                    ctypes.byref(o), ctypes.sizeof(o), ptr_of(col_order), stream(),
                                    ctypes.byref(h))
    return rc, h


def raw_info(h):
    info = _lib.PlanInfo()
    assert lib.maxk_plan_get_info_sized(h, ctypes.byref(info), ctypes.sizeof(info)) == 0
    fb, bb = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.maxk_plan_workspace_bytes(h, ctypes.byref(fb), ctypes.byref(bb)) == 0
    d = info.as_dict()
    d["fwd_workspace_bytes"], d["bwd_workspace_bytes"] = int(fb.value), int(bb.value)
    return d


def nonnull_arrays(info, opts):
    """The plan arrays that are non-null, from what the plan reports and was asked for
    (plan.hip: the stages plan_create_impl runs, each array taken through plan_alloc or
    plan_adopt)."""
    owned = not opts.get("external_workspace", 0)
    s = set()
    if info["fwd_tasks"] > 0:
        s |= {"fwd_tasks", "fwd_phase_off"}
        if info["num_edges"] > 0:
            s |= {"fwd_perm", "fwd_cv"}
        if info["fwd_fixed"]:
            s |= {"fwd_fix", "fwd_rowptr"}
    if info["fwd_split_rows"] > 0:
        s.add("zero_rows")
    if owned and info["fwd_workspace_bytes"] > 0:
        s.add("fwd_rec")
    if info["num_edges"] > 0:
        s.add("bwd_perm")
        if info["bwd_algo"] == _lib.BWD_ALGOS["two_pass"]:
            s |= {"bwd_erec", "bwd_colptr"}
            if info["bwd_tp_chunks"] > 1:
                s.add("bwd_colptr2")
            if owned and info["bwd_workspace_bytes"] > 0:
                s.add("bwd_tbuf")
        else:
            s.add("bwd_rec")
            if info["bwd_tasks"] > 0:
                s.add("bwd_tasks")
            if info["bwd_workspace_bytes"] > 0:      # the slabs of split blocks
                s.add("bwd_combine")
                if owned:
                    s.add("bwd_sel")
    if info["col_order"] in (_lib.COL_ORDERS["scattered"], _lib.COL_ORDERS["given"]):
        s.add("bwd_corder")
    return s


def check_case_shape(name, case, info, arrays):
    assert case["sets"] <= arrays, (name, sorted(case["sets"] - arrays))
    assert not (case.get("unset", set()) & arrays), (name, sorted(case["unset"] & arrays))
    if "layout" in case:
        assert info["fwd_layout"] == case["layout"], (name, info["fwd_layout"])
    tp = case.get("opts", {}).get("bwd_tp_chunks")
    if tp:
        assert info["bwd_tp_chunks"] == tp


# =========================================================================== accounting
ALL_CASES = dict(CASES, **SHAPE_CASES)


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_device_bytes_is_what_the_plan_holds(gpu, granule, big, name):
    """|held - device_bytes| <= (non-null arrays) x granule, both ways; destroy gives all of it
    back."""
    case = ALL_CASES[name]
    gr = big[case.get("graph", "uniform")]
    opts = resolved_options(case, gr)
    perm = gr.perm if case.get("given") else None

    def once():
        before = level()
        rc, h = raw_create(gr, case["k"], opts, perm)
        assert rc == 0, (name, rc, lib.maxk_last_error())
        held = before - level()
        info = raw_info(h)
        assert lib.maxk_plan_destroy(h) == 0
        return held, level() - (before - held), info

    RAN["accounting"].add(name)
    # warm-up: the stream-ordered pool of the build's scratch may keep a reserve (the slowest
    # case, seconds per build and no such scratch, goes without and waits measured()'s longest)
    wait = timed(once)[0] if case.get("warm_up", True) else 1.0
    held, back, info = measured(granule, once, wait)
    arrays = nonnull_arrays(info, opts)
    for a in arrays:
        COVERED.setdefault(a, []).append(name)
    slack = len(arrays) * granule
    reported = info["device_bytes"]
    ROWS.append((name, held, reported, slack, len(arrays)))
    print(f"\nplan lifetime: {name}: held {held} ({mib(held)}), device_bytes {reported} "
          f"({mib(reported)}), held - reported {held - reported}, slack {slack} "
          f"({len(arrays)} arrays)")
    check_case_shape(name, case, info, arrays)
    assert abs(held - reported) <= slack, \
        (f"{name}: the plan holds {held} bytes and reports {reported}: "
         f"{'under' if held > reported else 'over'}-reported by {abs(held - reported)}, slack {slack}")
    assert abs(back - held) <= granule, f"{name}: destroy gave back {back} of {held} bytes"
    if name in ("no_edges", "no_nodes"):          # both within one granule of zero
        assert 0 <= reported <= granule and abs(held) <= granule, (name, held, reported)


# =========================================================================== create/destroy
def cycle(gr, case, opts):
    """create -> forward -> backward -> refresh_values -> destroy."""
    k = case["k"]
    plan = mk.GraphPlan(gr.ptr, gr.idx, gr.val, gr.n, gr.e, D, k, num_cols=gr.nc, options=opts,
                        col_order=gr.perm if case.get("given") else None)
    info = plan.info()
    if gr.n > 0 and gr.nc > 0 and case.get("graph") != "tall":   # (tall: 10 GB of output)
        sp_data, sp_index, grad = gr.tables(k)
        plan.forward(sp_data, sp_index)
        plan.backward(grad, sp_index)
    plan.refresh_values(gr.val2)
    torch.cuda.synchronize()
    plan.__del__()
    assert not plan.handle.value
    RAN["cycles"] += 1
    return info


@pytest.mark.parametrize("name", list(CASES) + ["tall"])
def test_create_destroy_cycles_do_not_grow(gpu, granule, big, name):
    """One warm-up cycle, then 10: the free memory ends within one granule of where it was
    after the warm-up."""
    case = ALL_CASES[name]
    gr = big[case.get("graph", "uniform")]
    opts = resolved_options(case, gr)
    if gr.n and name != "tall":
        gr.tables(case["k"])
    one, info = timed(lambda: cycle(gr, case, opts))
    check_case_shape(name, case, info, nonnull_arrays(info, opts))

    def ten():
        base = level()
        for _ in range(CYCLES):
            cycle(gr, case, opts)
        return base - level()

    grown = measured(granule, ten, CYCLES * one)
    print(f"\nplan lifetime: {name}: {CYCLES} cycles, free memory fell by {grown} bytes")
    assert abs(grown) <= granule, f"{name}: {grown} bytes gone after {CYCLES} cycles"


# =========================================================================== oracle helpers
def numpy_graph(n, e, seed, limit=None, n1=0):
    """A small CSR graph (numpy): rows below n1 take their columns from [0, n1)."""
    rs = np.random.RandomState(seed)
    deg = rs.multinomial(e, np.ones(n) / n)
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    rows = np.repeat(np.arange(n), deg)
    hi = np.where(rows < n1, n1, n if limit is None else limit)
    idx = (rs.random_sample(e) * hi).astype(np.int32)
    val = rs.uniform(0.25, 1.0, e).astype(np.float32)
    return ptr, idx, val


def features(n, k, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, D)).astype(np.float32)
    g = rs.standard_normal((n, D)).astype(np.float32)
    od, oi = oracle.maxk(x, k)
    return x, g, od, oi


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def check_ops(dev, graph_t, graph_np, feats, k, what):
    """mk.spgemm_forward / mk.spgemm_backward without ``plan=`` against the oracle."""
    ptr, idx, val = graph_t
    p, ix, v = graph_np
    _, g, od, oi = feats
    n, e = p.size - 1, ix.size
    sd, si, gt = to(dev, od[:n], oi[:n], g[:n])
    y, _ = mk.spgemm_forward(ptr, idx, val, sd, si, n, e, k, D)
    gs = mk.spgemm_backward(ptr, idx, val, gt, si, n, e, k, D)
    ref, mag = oracle.spgemm_forward(p, ix, v, od[:n], oi[:n], D, with_mag=True)
    ok, worst = oracle.close_enough(y.cpu().numpy(), ref, mag)
    assert ok, f"{what}: forward worst err/bound {worst:.3g}"
    ref, mag = oracle.sspmm_backward(p, ix, v, g[:n], oi[:n], with_mag=True)
    ok, worst = oracle.close_enough(gs.cpu().numpy(), ref, mag)
    assert ok, f"{what}: backward worst err/bound {worst:.3g}"


@pytest.fixture
def creations(monkeypatch):
    """Counts maxk_plan_create_sized calls."""
    real = lib.maxk_plan_create_sized
    calls = []

    def counting(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(lib, "maxk_plan_create_sized", counting)
    mk.clear_plan_cache()
    yield calls
    mk.clear_plan_cache()


# =========================================================================== refused creates
REFUSALS = ["ptr_end", "col_order_repeat", "removed_option", "idx_past_end", "idx_negative"]


@pytest.mark.parametrize("how", REFUSALS)
def test_refused_creates_leak_nothing(gpu, granule, big, how):
    gr = big["uniform"]
    k = 16
    opts, perm, edges, want, code = {"external_workspace": 1}, None, None, None, -1
    if how == "ptr_end":                      # refused on the host after the copy of ptr
        edges, want = gr.e - 1, "ptr[N] must equal num_edges"
    elif how == "col_order_repeat":           # refused on the host after the first allocations
        perm = gr.perm.clone()
        perm[7] = perm[8]
        want = "not a permutation"
    elif how == "removed_option":             # refused before any device call
        opts["col_order"] = 3
        want, code = "removed in ABI 3", -2
    else:                                     # refused after the forward build and the block sort
        bad = Graph(gr.ptr, gr.idx.clone(), gr.val, gr.n, gr.nc)
        bad.idx[gr.e // 2] = gr.nc if how == "idx_past_end" else -1
        opts["col_order"] = 2
        gr, want = bad, "column ids outside"

    def refuse():
        rc, h = raw_create(gr, k, opts, perm, edges)
        assert rc == code and not h.value, (how, rc, h.value)
        assert want in lib.maxk_last_error().decode(), lib.maxk_last_error()
        RAN["refused"] += 1

    one = timed(refuse)[0]

    def ten():
        base = level()
        for _ in range(CYCLES):
            refuse()
        return base - level()

    grown = measured(granule, ten, CYCLES * one)
    print(f"\nplan lifetime: refused ({how}) x {CYCLES}: free memory fell by {grown} bytes")
    assert abs(grown) <= granule, f"{how}: {grown} bytes gone after {CYCLES} refused creates"


def test_good_plan_after_the_refusals(gpu):
    p, ix, v = numpy_graph(3000, 90_000, seed=21)
    mk.clear_plan_cache()
    check_ops(gpu, to(gpu, p, ix, v), (p, ix, v), features(3000, 16, 22), 16, "after refusals")
    mk.clear_plan_cache()


# =========================================================================== the cache, real plans
N_S, E_S, K_S = 3000, 90_000, 16
# where freed memory has to be seen coming back: every E-sized array above a granule (smaller
# ones are fragments of blocks they share with other plans' arrays)
N_M, E_M = 30_000, 1_200_000


def test_cache_same_address_other_graph(gpu, creations):
    """A graph deleted after ``clear_plan_cache()`` and another one allocated at the same
    addresses, with the same shapes and version counters: the whole key is equal, and only the
    cleared cache keeps the second graph from running on the first one's plan."""
    feats = features(N_S, K_S, 31)
    a_np = numpy_graph(N_S, E_S, seed=32)
    b_np = numpy_graph(N_S, E_S, seed=33)
    b_np = (a_np[0], b_np[1], b_np[2])        # equal shapes (and degrees), another structure
    assert not np.array_equal(a_np[1], b_np[1])
    torch.cuda.synchronize()
    a = to(gpu, *a_np)
    check_ops(gpu, a, a_np, feats, K_S, "graph A")
    assert len(creations) == 1
    old = tuple((t.data_ptr(), t._version) for t in a)
    mk.clear_plan_cache()
    del a
    b = to(gpu, *b_np)
    assert tuple((t.data_ptr(), t._version) for t in b) == old, \
        "graph B did not land on graph A's addresses: this test no longer tests anything"
    check_ops(gpu, b, b_np, feats, K_S, "graph B at A's addresses")
    assert len(creations) == 2


def test_cache_follows_inplace_edits(gpu, creations):
    feats = features(N_S, K_S, 41)
    p, ix, v = numpy_graph(N_S, E_S, seed=42)
    ix2 = (N_S - 1 - ix).astype(np.int32)
    g = to(gpu, p, ix, v)
    check_ops(gpu, g, (p, ix, v), feats, K_S, "before the edits")
    check_ops(gpu, g, (p, ix, v), feats, K_S, "a second call")
    assert len(creations) == 1
    g[1].copy_(torch.from_numpy(ix2))                      # another structure: a second plan
    check_ops(gpu, g, (p, ix2, v), feats, K_S, "after idx.copy_")
    assert len(creations) == 2
    g[2].mul_(0.5)                                         # other values: the same plan, refreshed
    check_ops(gpu, g, (p, ix2, v * np.float32(0.5)), feats, K_S, "after val.mul_")
    assert len(creations) == 2


def test_cache_prefix_subgraph_and_parent(gpu, creations):
    n1 = 1000
    feats = features(N_S, K_S, 51)
    p, ix, v = numpy_graph(N_S, E_S, seed=52, n1=n1)
    e1 = int(p[n1])
    g = to(gpu, p, ix, v)
    sub = (g[0][:n1 + 1], g[1][:e1], g[2][:e1])
    sub_np = (p[:n1 + 1], ix[:e1], v[:e1])
    assert sub[0].data_ptr() == g[0].data_ptr() and sub[1].data_ptr() == g[1].data_ptr()
    for turn in range(2):
        check_ops(gpu, g, (p, ix, v), feats, K_S, f"parent, turn {turn}")
        check_ops(gpu, sub, sub_np, feats, K_S, f"prefix sub-graph, turn {turn}")
    assert len(creations) == 2


def test_cache_byte_budget_with_real_plans(gpu, granule, creations, monkeypatch):
    """Three equal-sized graphs under a budget of 2.5 plans: two stay, the total is within the
    budget, and the evicted plan's memory is back."""
    p, ix, v = numpy_graph(N_M, E_M, seed=61)
    gs = [to(gpu, p, np.roll(ix, s), v) for s in (0, 1, 2)]
    torch.cuda.synchronize()
    one = ops.get_plan(*gs[0], N_M, E_M, D, K_S).device_bytes
    mk.clear_plan_cache()
    monkeypatch.setattr(ops, "_PLAN_CACHE_BYTES", int(2.5 * one))

    def fill():
        mk.clear_plan_cache()
        base = level()
        for g in gs[:2]:
            ops.get_plan(*g, N_M, E_M, D, K_S)
        two = base - level()
        assert len(ops._PLAN_CACHE) == 2 and ops.cached_plan_bytes() <= int(2.5 * one)
        ops.get_plan(*gs[2], N_M, E_M, D, K_S)
        return two, base - level()

    wait = timed(fill)[0]
    n0 = len(creations)
    two, three = measured(granule, fill, wait)
    print(f"\nplan lifetime: byte budget: one plan reports {one}; two plans hold {two}, after the "
          f"third {three}")
    built = len(creations) - n0
    assert built >= 3 and built % 3 == 0, built      # three builds per (repeated) measurement
    assert len(ops._PLAN_CACHE) == 2 and ops.cached_plan_bytes() <= int(2.5 * one)
    assert [pl._refs[1] is g[1] for pl, g in zip(ops._PLAN_CACHE.values(), gs[1:])] == [True, True]
    assert two >= granule and abs(three - two) <= granule, \
        f"two plans held {two} bytes, two plans after an eviction hold {three}"


# =========================================================================== autograd
@pytest.mark.parametrize("form", ["aggregate", "self_aggregate", "edge_weight"])
def test_backward_after_eviction_runs_on_a_live_plan(gpu, granule, monkeypatch, form):
    """The autograd context keeps its plan through eviction and ``clear_plan_cache()``: the
    backward is right, the plan's memory is held until the graph of ``y`` goes and is back
    afterwards."""
    k = K_S
    p, ix, v = numpy_graph(N_M, E_M, seed=71)
    p2, ix2, v2 = numpy_graph(N_M, E_M, seed=72)
    x, g, _, oi = features(N_M, k, 73)
    w = np.random.RandomState(74).uniform(0.5, 1.5, E_M).astype(np.float32)
    v_eff = (v * w).astype(np.float32) if form == "edge_weight" else v
    gs_ref, gs_mag = oracle.sspmm_backward(p, ix, v_eff, g, oi, with_mag=True)
    gx_ref, gx_mag = oracle.maxk_backward(gs_ref, oi, D), oracle.maxk_backward(gs_mag, oi, D)
    mk.clear_plan_cache()
    xt, gt, wt = to(gpu, x, g, w)
    other = mk.CSRGraph(*to(gpu, p2, ix2, v2))

    def step():
        mk.clear_plan_cache()
        graph = mk.CSRGraph(*to(gpu, p, ix, v))
        xr = xt.clone().requires_grad_(True)
        before = level()
        if form == "aggregate":
            y = mk.maxk_aggregate(xr, graph, k)
            plan = graph.plan(D, k)
        elif form == "self_aggregate":
            y = mk.maxk_self_aggregate(xr, graph, k)[1]   # (x_m would keep the context too)
            plan = graph.plan(D, k)
        else:
            y = mk.maxk_aggregate(xr, graph, k, edge_weight=wt)
            plan = graph.weighted_plan(D, k)
        reported = plan.device_bytes
        arrays = len(nonnull_arrays(plan.info(), {"external_workspace": 1}))
        del plan
        # force the plan out: a budget of one byte and another graph's plan, then the clear
        monkeypatch.setattr(ops, "_PLAN_CACHE_BYTES", 1)
        other.plan(D, k)
        assert len(ops._PLAN_CACHE) == 1 and next(iter(ops._PLAN_CACHE.values()))._refs[0] is other.ptr
        mk.clear_plan_cache()
        if form == "edge_weight":
            graph = None                        # the weighted plan lives on the graph object
        held = before - level()
        y.backward(gt)
        gx = xr.grad.cpu().numpy()
        still = before - level()
        del y
        after = before - level()
        return gx, reported, arrays, held, still, after

    # warm-up: the blocks that small arrays are fragments of stay with the runtime
    gx, reported, arrays, held, still, after = measured(granule, step, timed(step)[0])
    print(f"\nplan lifetime: {form}: plan reports {reported}; held after eviction {held}, after "
          f"backward {still}, after del y {after}")
    ok, worst = oracle.close_enough(gx, gx_ref, gx_mag)
    assert ok, f"{form}: x.grad after eviction, worst err/bound {worst:.3g}"
    slack = arrays * granule
    assert abs(held - reported) <= slack and abs(still - reported) <= slack, \
        f"{form}: the evicted plan should still hold {reported} bytes: {held}, {still}"
    assert abs(after) <= granule, f"{form}: {after} bytes still held after del y"
    mk.clear_plan_cache()


def test_plan_dropped_right_after_launch(gpu):
    """free_plan releases every array with a blocking hipFree, so dropping the last reference
    right after a launch on a side stream is safe; the autograd path relies on it."""
    k = K_S
    p, ix, v = numpy_graph(N_S, E_S, seed=81)
    _, _, od, oi = features(N_S, k, 82)
    ref, mag = oracle.spgemm_forward(p, ix, v, od, oi, D, with_mag=True)
    ptr, idx, val, sd, si = to(gpu, p, ix, v, od, oi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    plan = mk.GraphPlan(ptr, idx, val, N_S, E_S, D, k)
    with torch.cuda.stream(side):
        out = plan.forward(sd, si)
        del plan
    side.synchronize()
    ok, worst = oracle.close_enough(out.cpu().numpy(), ref, mag)
    assert ok, f"forward of a plan dropped right after launch: worst err/bound {worst:.3g}"


# =========================================================================== what ran
def test_plan_lifetime_report(gpu, granule):
    """Runs last (file order): the table of held memory against reported bytes, and that the
    accounting cases made every one of the 18 plan arrays non-null at least once."""
    if RAN["accounting"] != set(ALL_CASES):     # (a case that started and failed still counts)
        pytest.skip("not every accounting case was selected in this session (-k)")
    print(f"\nplan lifetime: granule {granule} bytes")
    print(f"{'case':<22}{'held':>14}{'device_bytes':>14}{'held-reported':>15}{'slack':>12} arrays")
    for name, held, reported, slack, n in ROWS:
        print(f"{name:<22}{held:>14}{reported:>14}{held - reported:>15}{slack:>12} {n}")
    for a in ARRAYS:
        print(f"plan lifetime: {a}: {', '.join(COVERED.get(a, [])) or 'NOT COVERED'}")
    missing = [a for a in ARRAYS if a not in COVERED]
    assert not missing, f"plan arrays no accounting case made non-null: {missing}"
    print(f"plan lifetime: all {len(ARRAYS)} plan arrays were covered; {RAN['cycles']} "
          f"create/destroy cycles and {RAN['refused']} refused creates ran; "
          f"{time.time() - T0:.0f} s since the module was imported")
