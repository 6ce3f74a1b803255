"""CPU: the policy of ``ops.get_plan`` (which plan a call runs on, what the cache keeps) and
``GraphPlan.__del__``, with the plan itself stubbed.

``ops.GraphPlan`` is replaced by a stub that records each construction, carries ``_refs`` and
``val_version`` like the real one, has a settable ``device_bytes`` and counts
``refresh_values``; the graph tensors are CPU tensors (the key reads only ``device.index``,
``data_ptr()`` and ``_version``). ``ops._PLAN_CACHE_BYTES`` is monkeypatched: the environment
variable is read at import and the default budget asks the device.

Every component of the key has a test of its own that differs from a cached call in that
component alone, so a key that drops one serves a stale plan in exactly that test: ``ptr`` /
``idx`` / ``val`` addresses, the ``ptr`` / ``idx`` version counters, N, E, D, k and the device
index (through a ``ptr`` stand-in that reports another index; real multi-device caches are
not covered).
"""
import ctypes
import threading
import types

import pytest
import torch

from maxk_kernels import ops

N, E, D, K = 6, 12, 32, 8
HUGE = 1 << 60


class StubPlan:
    """Stands in for ``ops.GraphPlan`` in ``get_plan``."""

    built = []          # every construction, in order
    next_bytes = 100    # device_bytes of the next plan built
    fail = None         # an exception to raise from the next construction
    on_build = None     # called at the start of a construction

    def __init__(self, ptr, idx, val, num_nodes, num_edges, dim_origin, dim_k):
        if StubPlan.on_build is not None:
            StubPlan.on_build()
        if StubPlan.fail is not None:
            raise StubPlan.fail
        self._refs = (ptr, idx, val)
        self.val_version = val._version
        self.args = (num_nodes, num_edges, dim_origin, dim_k)
        self.device_bytes = StubPlan.next_bytes
        self.refreshed = []
        StubPlan.built.append(self)

    def refresh_values(self, val):
        self.refreshed.append(val)
        self._refs = (self._refs[0], self._refs[1], val)
        self.val_version = val._version


@pytest.fixture
def cache(monkeypatch):
    ops.clear_plan_cache()
    StubPlan.built, StubPlan.next_bytes, StubPlan.fail, StubPlan.on_build = [], 100, None, None
    monkeypatch.setattr(ops, "GraphPlan", StubPlan)
    monkeypatch.setattr(ops, "_PLAN_CACHE_BYTES", HUGE)
    yield StubPlan
    ops.clear_plan_cache()
    StubPlan.built, StubPlan.fail, StubPlan.on_build = [], None, None


def graph(n=N, e=E, seed=0):
    g = torch.Generator().manual_seed(seed)
    ptr = torch.linspace(0, e, n + 1).to(torch.int32)
    idx = torch.randint(0, n, (e,), generator=g, dtype=torch.int32)
    val = torch.rand(e, generator=g)
    return ptr, idx, val


def cached():
    return list(ops._PLAN_CACHE.values())


# -------------------------------------------------------------------------------------------
# hit, and a miss on every component of the key
# -------------------------------------------------------------------------------------------
def test_hit_returns_the_same_plan_without_building(cache):
    ptr, idx, val = graph()
    a = ops.get_plan(ptr, idx, val, N, E, D, K)
    b = ops.get_plan(ptr, idx, val, N, E, D, K)
    assert a is b and cache.built == [a]
    assert a.args == (N, E, D, K) and a._refs[0] is ptr and a._refs[1] is idx and a._refs[2] is val
    assert a.refreshed == []


def _miss(cache, first, second):
    """``second`` differs from ``first`` in one key component: two plans, and each call gets
    its own again afterwards."""
    a = ops.get_plan(*first)
    b = ops.get_plan(*second)
    assert a is not b and cache.built == [a, b]
    assert ops.get_plan(*first) is a and ops.get_plan(*second) is b
    assert cache.built == [a, b] and a.refreshed == [] and b.refreshed == []
    return a, b


def test_miss_on_another_dim_origin(cache):
    ptr, idx, val = graph()
    a, b = _miss(cache, (ptr, idx, val, N, E, D, K), (ptr, idx, val, N, E, D + 32, K))
    assert a.args[2] == D and b.args[2] == D + 32


def test_miss_on_another_k(cache):
    ptr, idx, val = graph()
    a, b = _miss(cache, (ptr, idx, val, N, E, D, K), (ptr, idx, val, N, E, D, K + 8))
    assert a.args[3] == K and b.args[3] == K + 8


def test_miss_on_another_val_tensor(cache):
    ptr, idx, val = graph()
    val2 = val.clone()
    assert val2.data_ptr() != val.data_ptr()
    a, b = _miss(cache, (ptr, idx, val, N, E, D, K), (ptr, idx, val2, N, E, D, K))
    assert a._refs[2] is val and b._refs[2] is val2


def test_miss_on_another_ptr_tensor(cache):
    ptr, idx, val = graph()
    ptr2 = ptr.clone()
    assert ptr2.data_ptr() != ptr.data_ptr()
    a, b = _miss(cache, (ptr, idx, val, N, E, D, K), (ptr2, idx, val, N, E, D, K))
    assert a._refs[0] is ptr and b._refs[0] is ptr2


def test_miss_on_another_idx_tensor(cache):
    ptr, idx, val = graph()
    idx2 = idx.clone()
    assert idx2.data_ptr() != idx.data_ptr()
    a, b = _miss(cache, (ptr, idx, val, N, E, D, K), (ptr, idx2, val, N, E, D, K))
    assert a._refs[1] is idx and b._refs[1] is idx2


class OnDevice:
    """A ``ptr`` that reports another device index: what ``get_plan`` reads of it, no more."""

    def __init__(self, tensor, index):
        self._tensor = tensor
        self.device = types.SimpleNamespace(index=index)

    def data_ptr(self):
        return self._tensor.data_ptr()

    @property
    def _version(self):
        return self._tensor._version


def test_miss_on_another_device_index(cache):
    """Two devices can hand out the same address: the device index is part of the key."""
    ptr, idx, val = graph()
    p0, p1 = OnDevice(ptr, 0), OnDevice(ptr, 1)
    a, b = _miss(cache, (p0, idx, val, N, E, D, K), (p1, idx, val, N, E, D, K))
    assert a._refs[0] is p0 and b._refs[0] is p1


def test_miss_on_a_prefix_view(cache):
    """A sub-graph of the first n1 rows: the same addresses, other N and E."""
    ptr, idx, val = graph()
    n1 = 3
    e1 = int(ptr[n1])
    p1, i1, v1 = ptr[:n1 + 1], idx[:e1], val[:e1]
    assert (p1.data_ptr(), i1.data_ptr(), v1.data_ptr()) == \
        (ptr.data_ptr(), idx.data_ptr(), val.data_ptr())
    a, b = _miss(cache, (ptr, idx, val, N, E, D, K), (p1, i1, v1, n1, e1, D, K))
    assert a.args[:2] == (N, E) and b.args[:2] == (n1, e1)


def test_miss_on_num_nodes_alone(cache):
    """Trailing rows without edges: the same storage and E, another N."""
    ptr, idx, val = graph()
    ptr[-1] = ptr[-2]    # (before any plan: the version counter is the same for both calls)
    e = int(ptr[-1])
    assert ptr[:N].data_ptr() == ptr.data_ptr() and int(ptr[N - 1]) == e
    _miss(cache, (ptr, idx[:e], val[:e], N, e, D, K), (ptr[:N], idx[:e], val[:e], N - 1, e, D, K))


def test_miss_on_num_edges_alone(cache):
    """The key holds E on its own (the stub does not check it against ptr)."""
    ptr, idx, val = graph()
    _miss(cache, (ptr, idx, val, N, E, D, K), (ptr, idx, val, N, E - 1, D, K))


@pytest.mark.parametrize("which", ["idx", "ptr"])
def test_miss_on_a_versioned_inplace_edit_of_the_structure(cache, which):
    ptr, idx, val = graph()
    a = ops.get_plan(ptr, idx, val, N, E, D, K)
    if which == "idx":
        idx.copy_(graph(seed=1)[1])
    else:
        ptr.copy_(torch.arange(N + 1, dtype=torch.int32) * 2)
    b = ops.get_plan(ptr, idx, val, N, E, D, K)
    assert b is not a and cache.built == [a, b]
    assert ops.get_plan(ptr, idx, val, N, E, D, K) is b and cache.built == [a, b]


def test_inplace_edit_of_val_refreshes_once(cache):
    ptr, idx, val = graph()
    a = ops.get_plan(ptr, idx, val, N, E, D, K)
    val.mul_(2)
    assert ops.get_plan(ptr, idx, val, N, E, D, K) is a
    assert len(a.refreshed) == 1 and a.refreshed[0] is val
    assert ops.get_plan(ptr, idx, val, N, E, D, K) is a
    assert len(a.refreshed) == 1 and cache.built == [a]


# -------------------------------------------------------------------------------------------
# eviction
# -------------------------------------------------------------------------------------------
def test_lru_by_count(cache):
    ptr, idx, val = graph()
    size = ops._PLAN_CACHE_SIZE
    assert size == 32
    plans = [ops.get_plan(ptr, idx, val, N, E, d, K) for d in range(1, size + 1)]
    assert cached() == plans
    p33 = ops.get_plan(ptr, idx, val, N, E, size + 1, K)
    assert cached() == plans[1:] + [p33]                    # the oldest went
    # a hit moves its key to the young end: the next eviction takes another
    assert ops.get_plan(ptr, idx, val, N, E, 2, K) is plans[1]
    p34 = ops.get_plan(ptr, idx, val, N, E, size + 2, K)
    assert cached() == plans[3:] + [p33, plans[1], p34]     # plans[2] went, not plans[1]
    assert len(cache.built) == size + 2


def test_byte_budget_evicts_oldest_first(cache, monkeypatch):
    ptr, idx, val = graph()
    monkeypatch.setattr(ops, "_PLAN_CACHE_BYTES", 1000)
    sizes = [300, 300, 300]
    plans = []
    for d, b in enumerate(sizes, 1):
        cache.next_bytes = b
        plans.append(ops.get_plan(ptr, idx, val, N, E, d, K))
    assert cached() == plans and ops.cached_plan_bytes() == 900
    cache.next_bytes = 500                                   # 1400: two go until 800 fits
    p4 = ops.get_plan(ptr, idx, val, N, E, 4, K)
    assert cached() == [plans[2], p4]
    assert ops.cached_plan_bytes() == 800 == sum(p.device_bytes for p in cached())
    cache.next_bytes = 200                                   # exactly the budget: all stay
    p5 = ops.get_plan(ptr, idx, val, N, E, 5, K)
    assert cached() == [plans[2], p4, p5] and ops.cached_plan_bytes() == 1000
    cache.next_bytes = 1                                     # one byte over: the oldest goes
    p6 = ops.get_plan(ptr, idx, val, N, E, 6, K)
    assert cached() == [p4, p5, p6] and ops.cached_plan_bytes() == 701


def test_a_plan_larger_than_the_budget_stays(cache, monkeypatch):
    ptr, idx, val = graph()
    monkeypatch.setattr(ops, "_PLAN_CACHE_BYTES", 1000)
    small = ops.get_plan(ptr, idx, val, N, E, 1, K)
    cache.next_bytes = 5000
    big = ops.get_plan(ptr, idx, val, N, E, 2, K)
    assert cached() == [big] and ops.cached_plan_bytes() == 5000     # the len > 1 floor
    assert ops.get_plan(ptr, idx, val, N, E, 2, K) is big and cache.built == [small, big]
    cache.next_bytes = 10
    tiny = ops.get_plan(ptr, idx, val, N, E, 3, K)
    assert cached() == [tiny] and ops.cached_plan_bytes() == 10


def test_clear_plan_cache(cache):
    ptr, idx, val = graph()
    a = ops.get_plan(ptr, idx, val, N, E, D, K)
    ops.clear_plan_cache()
    assert cached() == [] and ops.cached_plan_bytes() == 0
    assert ops.get_plan(ptr, idx, val, N, E, D, K) is not a


# -------------------------------------------------------------------------------------------
# failure and threads
# -------------------------------------------------------------------------------------------
def test_construction_failure_leaves_the_cache_and_the_lock(cache):
    ptr, idx, val = graph()
    a = ops.get_plan(ptr, idx, val, N, E, D, K)
    before = list(ops._PLAN_CACHE.items())
    cache.fail = RuntimeError("no plan today")
    with pytest.raises(RuntimeError, match="no plan today"):
        ops.get_plan(ptr, idx, val, N, E, D + 1, K)
    assert list(ops._PLAN_CACHE.items()) == before
    assert ops._PLAN_LOCK.acquire(blocking=False)
    ops._PLAN_LOCK.release()
    cache.fail = None
    b = ops.get_plan(ptr, idx, val, N, E, D + 1, K)
    assert cached() == [a, b] and cache.built == [a, b]
    assert ops.get_plan(ptr, idx, val, N, E, D, K) is a


def test_eight_threads_build_one_plan(cache):
    ptr, idx, val = graph()
    nthreads = 8
    arrived, all_here, count_lock = [0], threading.Event(), threading.Lock()

    def on_build():
        # the build ends only once every thread is at (or past) its get_plan call, so without
        # the cache's lock the others would find no plan yet and build their own
        assert all_here.wait(timeout=30)

    cache.on_build = on_build
    got, errors = [None] * nthreads, []

    def worker(i):
        try:
            with count_lock:
                arrived[0] += 1
                if arrived[0] == nthreads:
                    all_here.set()
            got[i] = ops.get_plan(ptr, idx, val, N, E, D, K)
        except BaseException as exc:  # noqa: BLE001 - reported below
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not errors and not any(t.is_alive() for t in threads)
    assert len(cache.built) == 1 and all(g is cache.built[0] for g in got)


# -------------------------------------------------------------------------------------------
# GraphPlan.__del__ (the real class, the library stubbed)
# -------------------------------------------------------------------------------------------
class StubLib:
    def __init__(self):
        self.destroyed = []

    def maxk_plan_destroy(self, handle):
        self.destroyed.append(handle.value)
        return 0


def test_del_destroys_a_live_handle_exactly_once(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(ops, "lib", stub)
    plan = object.__new__(ops.GraphPlan)
    plan.handle = ctypes.c_void_p(0x1234)
    plan.__del__()
    assert stub.destroyed == [0x1234] and not plan.handle.value
    plan.__del__()
    assert stub.destroyed == [0x1234]
    del plan                                     # the collector's own call does nothing more
    assert stub.destroyed == [0x1234]


def test_del_ignores_a_null_handle(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(ops, "lib", stub)
    plan = object.__new__(ops.GraphPlan)
    plan.handle = ctypes.c_void_p(0)             # a create the library refused
    plan.__del__()
    del plan
    assert stub.destroyed == []


def test_del_after_init_raised_before_a_handle_existed(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(ops, "lib", stub)

    def refuse(*_):
        raise RuntimeError("refused before the handle")

    monkeypatch.setattr(ops, "_refuse_capture", refuse)
    ptr, idx, val = graph()
    with pytest.raises(RuntimeError, match="refused before the handle"):
        ops.GraphPlan(ptr, idx, val, N, E, D, K)
    bare = object.__new__(ops.GraphPlan)         # no attribute at all
    assert not hasattr(bare, "handle")
    bare.__del__()
    del bare
    assert stub.destroyed == []
