"""CPU: the neighbour-sampling entry points are declared, bound and refuse bad arguments on the
host (null or made-up device pointers: nothing reaches a GPU); the numpy restatements of
tests/sampling.py hold the properties the rule promises; the hash is uniform enough; the test
graphs hold the preconditions of the GPU cases; the maxk_sp:: fixture is the library's set; and
Block and the layers behave on the host as documented."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import maxk_kernels as mk
import sampling as sp
from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_sample.txt")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

NEW = ("maxk_sample_neighbors", "maxk_sample_scratch_bytes", "maxk_sample_row_limits",
       "maxk_block_compact", "maxk_block_compact_scratch_bytes")
P = ctypes.c_void_p
lib = _lib.lib
INVALID = -1
I32MAX = 2 ** 31 - 1
BASE = 1 << 20


def err():
    return lib.maxk_last_error().decode()


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "Neighbour sampling (ABI 4)" in open(HEADER).read()
    assert lib.maxk_abi_version() == 4
    for name in ("sample_neighbors", "block_compact", "Block", "NeighborSampler", "to_block",
                 "block_aggregate", "block_self_aggregate", "sample_row_limits", "layer_seed"):
        assert name in mk.__all__ and hasattr(mk, name), name
    from maxk_kernels import ops
    assert callable(ops.sample_neighbors) and callable(ops.block_compact)


def test_row_limits_and_scratch_sizes():
    assert lib.maxk_sample_row_limits(None, 0) == 2
    buf = (ctypes.c_int32 * 4)(*([-7] * 4))
    assert lib.maxk_sample_row_limits(ctypes.cast(buf, P), 1) == 2
    assert list(buf) == [sp.LIMITS[0], -7, -7, -7]
    assert lib.maxk_sample_row_limits(ctypes.cast(buf, P), 4) == 2
    assert tuple(buf[:2]) == sp.LIMITS and buf[2] == -7
    assert mk.sample_row_limits() == sp.LIMITS
    for n in (0, 1, 2046, 2047, 2048, 65536, 10 ** 6):
        assert lib.maxk_sample_scratch_bytes(n) == sp.sample_scratch_bytes(n), n
        assert lib.maxk_block_compact_scratch_bytes(n) == sp.compact_scratch_bytes(n), n
    assert lib.maxk_sample_scratch_bytes(-1) == 0 and lib.maxk_block_compact_scratch_bytes(-3) == 0


# ------------------------------------------------------------------ refusals
def sample(ptr=P(BASE), idx=P(BASE + (1 << 16)), seeds=P(BASE + (2 << 16)),
           out_ptr=P(BASE + (3 << 16)), col=P(BASE + (4 << 16)), eid=P(BASE + (5 << 16)),
           cap=1000, scratch=P(BASE + (6 << 16)), sb=None, n=100, e=5000, s=100, fanout=10,
           seed=1):
    sb = sp.sample_scratch_bytes(max(s, 0)) if sb is None else sb
    return lib.maxk_sample_neighbors(ptr, idx, seeds, out_ptr, col, eid, cap, scratch, sb, n, e,
                                     s, fanout, seed, None)


def compact(seeds=P(BASE), cols=P(BASE + (1 << 16)), src=P(BASE + (2 << 16)), cap=1100,
            local=P(BASE + (3 << 16)), counts=P(BASE + (4 << 16)), scratch=P(BASE + (5 << 16)),
            sb=None, s=100, m=1000, nc=600):
    sb = sp.compact_scratch_bytes(max(nc, 0)) if sb is None else sb
    return lib.maxk_block_compact(seeds, cols, src, cap, local, counts, scratch, sb, s, m, nc,
                                  None)


SAMPLE_REFUSALS = [
    (dict(fanout=0), "fanout"),
    (dict(s=-1), "negative number of seeds"),
    (dict(n=-1), "sizes"), (dict(e=-1), "sizes"), (dict(e=I32MAX + 1), "sizes"),
    (dict(cap=I32MAX + 1), "fit int32"), (dict(cap=-1), "fit int32"),
    (dict(n=0), "seeds without rows"),
    (dict(sb=8), "scratch_bytes"),
    (dict(ptr=None), "null pointer"), (dict(idx=None), "null pointer"),
    (dict(seeds=None), "null pointer"), (dict(out_ptr=None), "null pointer"),
    (dict(col=None), "null pointer"), (dict(eid=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(col=P(BASE + 4)), "overlaps"), (dict(eid=P(BASE + (1 << 16) + 4)), "overlaps"),
    (dict(out_ptr=P(BASE + (2 << 16) + 4)), "overlaps"),
    (dict(eid=P(BASE + (4 << 16) + 8)), "overlaps"),
    (dict(scratch=P(BASE + (3 << 16) + 4)), "overlaps"),
]


@pytest.mark.parametrize("kw,msg", SAMPLE_REFUSALS)
def test_sampler_refusals_on_the_host(kw, msg):
    got = sample(**kw)
    assert got == INVALID, (kw, got, err())
    assert msg in err(), err()


COMPACT_REFUSALS = [
    (dict(s=-1), "sizes"), (dict(m=-1), "sizes"), (dict(nc=-1), "sizes"),
    (dict(m=I32MAX + 1), "sizes"), (dict(cap=I32MAX + 1), "fit int32"),
    (dict(nc=0), "without columns"), (dict(cap=99), "hold the seeds"),
    (dict(sb=100), "scratch_bytes"),
    (dict(seeds=None), "null pointer"), (dict(cols=None), "null pointer"),
    (dict(src=None), "null pointer"), (dict(local=None), "null pointer"),
    (dict(counts=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(src=P(BASE + 4)), "overlaps"), (dict(local=P(BASE + (1 << 16) + 4)), "overlaps"),
    (dict(counts=P(BASE + (2 << 16) + 4)), "overlaps"),
    (dict(scratch=P(BASE + (3 << 16) + 4)), "overlaps"),
]


@pytest.mark.parametrize("kw,msg", COMPACT_REFUSALS)
def test_compaction_refusals_on_the_host(kw, msg):
    got = compact(**kw)
    assert got == INVALID, (kw, got, err())
    assert msg in err(), err()


# ------------------------------------------------------------------ the restatement
def fmix32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_hash_is_the_composition_of_the_header():
    text = open(HEADER).read()
    assert "key(e)  = fmix32(fmix32(e ^ lo) ^ fmix32(e * 0x9E3779B1 + hi))" in text
    assert "rank(e) = (uint64)key(e) << 32 | e" in text
    for seed in (0, 1, 0xDEADBEEF, 0x0123456789ABCDEF, 2 ** 64 - 1):
        lo, hi = seed & 0xFFFFFFFF, seed >> 32
        for e in (0, 1, 199, 2 ** 31 - 1):
            want = fmix32_int(fmix32_int(e ^ lo) ^ fmix32_int(e * 0x9E3779B1 + hi))
            assert int(sp.edge_key(seed, [e])[0]) == want, (seed, e)
            assert int(sp.edge_rank(seed, [e])[0]) == (want << 32 | e)
    # a seed is taken modulo 2^64, and the high word matters
    assert np.array_equal(sp.edge_key(-1, np.arange(50)), sp.edge_key(2 ** 64 - 1, np.arange(50)))
    assert not np.array_equal(sp.edge_key(7, np.arange(50)), sp.edge_key(7 + (1 << 32), np.arange(50)))


@pytest.mark.parametrize("name", sorted(sp.GRAPHS))
def test_selection_and_compaction_properties(name):
    ptr, idx, num_cols = sp.GRAPHS[name]()
    n = ptr.size - 1
    lens = np.diff(ptr)
    sets = sp.seed_sets(ptr)
    for fanout in (2, 25, -1):
        out_ptr, col, eid = sp.sample_ref(ptr, idx, sets["all"], fanout, seed=11)
        want = lens if fanout < 0 else np.minimum(lens, fanout)
        assert np.array_equal(np.diff(out_ptr), want) and out_ptr[0] == 0
        assert np.array_equal(col, idx[eid])
        for r in (0, sp.hub_row(ptr), n - 1, 17):
            mine = eid[out_ptr[r]:out_ptr[r + 1]].astype(np.int64)
            assert (np.diff(mine) > 0).all() and ((mine >= ptr[r]) & (mine < ptr[r + 1])).all()
            rest = np.setdiff1d(np.arange(ptr[r], ptr[r + 1]), mine)
            if rest.size and mine.size:  # every kept rank lies below every dropped one
                assert sp.edge_rank(11, mine).max() < sp.edge_rank(11, rest).min()
        # a row's sample does not depend on the batch or on its place in it
        perm = sets["permutation"]
        p_ptr, p_col, p_eid = sp.sample_ref(ptr, idx, perm, fanout, seed=11)
        for i in (0, 5, n - 1):
            r = perm[i]
            assert np.array_equal(p_eid[p_ptr[i]:p_ptr[i + 1]], eid[out_ptr[r]:out_ptr[r + 1]])
        # compaction
        for seeds in (sets["all"], perm[:37], sets["hub"], sets["none"]):
            s_ptr, s_col, _ = sp.sample_ref(ptr, idx, seeds, fanout, seed=11)
            src, local, (num_src, distinct) = sp.compact_ref(seeds, s_col, num_cols)
            assert distinct == len(seeds) and num_src == src.size == np.unique(src).size
            assert np.array_equal(src[:len(seeds)], seeds)
            assert (np.diff(src[len(seeds):]) > 0).all()
            assert np.array_equal(src[local], s_col) if s_col.size else local.size == 0
            assert set(src[len(seeds):].tolist()) == set(s_col.tolist()) - set(seeds.tolist())
    src, local, counts = sp.compact_ref(np.array([4, 9, 4]), np.array([9, 4, 2]), num_cols)
    assert counts == (4, 2) and src.tolist() == [4, 9, 4, 2] and local.tolist() == [1, 0, 3]


def test_graphs_hold_the_preconditions_of_the_gpu_cases():
    """Rows of length 0, 1, f - 1, f, f + 1 for every fanout used, rows on both sides of every
    limit the library reports (and at it), every regime, and more columns than rows in the
    rectangular graph."""
    assert mk.sample_row_limits() == sp.LIMITS
    rect_ptr, rect_idx, rect_cols = sp.rect_graph()
    sq_ptr, _, sq_cols = sp.square_graph()
    assert rect_cols > rect_ptr.size - 1 and sq_cols == sq_ptr.size - 1 == 600
    assert rect_idx.max() >= rect_ptr.size - 1     # columns past the row count are in use
    rect_lens, both = set(np.diff(rect_ptr).tolist()), set(np.diff(sq_ptr).tolist())
    both |= rect_lens
    need = {0, 1}
    for f in sp.FANOUTS:
        need |= {f - 1, f, f + 1}
    for limit in sp.LIMITS:
        need |= {limit - 1, limit, limit + 1}
    assert need <= rect_lens, sorted(need - rect_lens)
    assert {sp.regime(n) for n in np.diff(sq_ptr)} == {0, 1, 2} == {sp.regime(n) for n in rect_lens}
    assert np.diff(sq_ptr).max() == 5000
    for ptr in (rect_ptr, sq_ptr):
        big = sp.fanouts_for(ptr)[-2]
        assert big > np.diff(ptr).max() and sp.fanouts_for(ptr)[-1] == -1
        sets = sp.seed_sets(ptr)
        assert np.diff(ptr)[sets["empty_row"][0]] == 0 and sets["none"].size == 0
        assert sorted(sets["permutation"].tolist()) == list(range(ptr.size - 1))
        assert not np.array_equal(sets["permutation"], sets["all"])
    # rows that need a selection exist in every regime for some fanout used
    for lo, hi in ((2, 16), (17, 512), (513, 10 ** 9)):
        assert any(lo <= n <= hi and n > 1 for n in both)


def test_uniformity_of_the_chosen_hash():
    """A 200-edge row, fanout 10, seeds 0 .. 4095: every edge's inclusion count lies within 5
    standard deviations of the binomial mean, and no pair of adjacent edges is kept together more
    often than 5 standard deviations above its mean. Deterministic: a property of the rule."""
    n, f, trials = 200, 10, 4096
    for b in (0, 12345):
        inc, pair = np.zeros(n), np.zeros(n - 1)
        for seed in range(trials):
            m = np.zeros(n, bool)
            m[sp.kept_edges(b, n, f, seed) - b] = True
            assert m.sum() == f
            inc += m
            pair += m[1:] & m[:-1]
        p = f / n
        mu, sd = trials * p, (trials * p * (1 - p)) ** 0.5
        assert (np.abs(inc - mu) <= 5 * sd).all(), (b, inc.min(), inc.max(), mu, sd)
        pp = f * (f - 1) / (n * (n - 1))
        pmu, psd = trials * pp, (trials * pp * (1 - pp)) ** 0.5
        assert pair.max() <= pmu + 5 * psd, (b, pair.max(), pmu, psd)


def test_tie_break_case_exists_and_is_decided_by_the_edge_number():
    seed, fanout, e0, e1 = sp.tie_break_case()
    ptr, idx, _ = sp.square_graph()
    r = sp.hub_row(ptr)
    assert ptr[r] <= e0 < e1 < ptr[r + 1] and 0 < fanout < ptr[r + 1] - ptr[r]
    assert sp.edge_key(seed, [e0])[0] == sp.edge_key(seed, [e1])[0]
    kept = sp.kept_edges(int(ptr[r]), int(ptr[r + 1] - ptr[r]), fanout, seed)
    assert e0 in kept and e1 not in kept and kept.size == fanout
    more = sp.kept_edges(int(ptr[r]), int(ptr[r + 1] - ptr[r]), fanout + 1, seed)
    assert e1 in more
    # the threshold falls between them: e0 holds the highest kept rank
    assert sp.edge_rank(seed, kept).max() == sp.edge_rank(seed, [e0])[0]


# ------------------------------------------------------------------ selectors, fixtures
def test_restated_names_cover_the_fixture():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_sp::") for n in names)
    restated = set(sp.KERNELS) | {sp.sample_kernel_name(f) for f in (-1, 1, 10, 2 ** 31 - 1)}
    assert restated == set(names) and len(names) == 7
    assert set(sp.SAMPLER_KERNELS) | set(sp.COMPACT_KERNELS) == set(sp.KERNELS) | set(sp.SCAN_KERNELS)
    assert all(n.startswith("maxk_scan::") for n in sp.SCAN_KERNELS)


def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_sp::") == kernel_list.read_list(FIXTURE)
    assert kernel_list.main([_lib.LIB_PATH, "--namespace", "maxk_sp::", "--diff", FIXTURE]) == 0


# ------------------------------------------------------------------ Block, sampler, layers
def hand_block():
    # 3 destinations over 5 sources; row 1 is empty; column 4 twice in row 2
    return mk.Block(torch.tensor([0, 2, 2, 5]), torch.tensor([1, 3, 0, 4, 4]),
                    torch.tensor([2.0, 3.0, 5.0, 7.0, 11.0]), num_src=5,
                    src_ids=torch.tensor([10, 20, 30, 7, 8], dtype=torch.int32),
                    eids=torch.tensor([3, 4, 9, 11, 12], dtype=torch.int32))


def test_block_invariants():
    b = hand_block()
    assert isinstance(b, mk.CSRGraph) and (b.num_dst, b.num_src, b.num_edges) == (3, 5, 5)
    assert b.num_nodes == 3 and b.dst_ids.tolist() == [10, 20, 30]
    assert b.ptr.dtype == b.idx.dtype == torch.int32 and b.val.dtype == torch.float32
    assert b.in_degrees().tolist() == [2, 0, 3]
    assert b.out_degrees().tolist() == [1, 1, 0, 1, 2]
    assert b.edge_values("sum").tolist() == [1.0] * 5
    third = float(np.float32(1) / np.float32(3))
    assert b.edge_values("mean").tolist() == [0.5, 0.5, third, third, third]
    m = b.with_values("mean")
    assert isinstance(m, mk.Block) and m is b.with_values("mean") and m.num_src == 5
    assert m.ptr is b.ptr and m.idx is b.idx and m.src_ids is b.src_ids and m.eids is b.eids
    assert torch.equal(m.val, b.edge_values("mean")) and b.val.tolist() == [2, 3, 5, 7, 11]
    ptr_t, idx_t, order = b.transposed_structure()
    assert ptr_t.tolist() == [0, 1, 2, 2, 3, 5] and idx_t.tolist() == [2, 0, 0, 2, 2]
    assert order.tolist() == [2, 0, 1, 3, 4] and ptr_t.dtype == idx_t.dtype == torch.int32
    assert b.transposed_order().tolist() == order.tolist()
    assert b.transposed_order().dtype == torch.int32
    t = b.transposed()
    assert (t.num_nodes, t.num_src) == (5, 3) and t.ptr.tolist() == ptr_t.tolist()
    assert t.idx.tolist() == idx_t.tolist() and t.val.tolist() == [5, 2, 3, 7, 11]
    # nothing changes for a plain CSRGraph
    g = mk.CSRGraph(torch.tensor([0, 2, 2, 5]), torch.tensor([1, 2, 0, 2, 2]))
    assert g.out_degrees().tolist() == [1, 1, 3] and g.transposed_structure()[0].numel() == 4
    assert type(g.with_values("mean")) is mk.CSRGraph


def test_layer_seed_rule_and_sampler_arguments():
    def fmix64(x):
        x &= 2 ** 64 - 1
        x ^= x >> 33
        x = (x * 0xFF51AFD7ED558CCD) % 2 ** 64
        x ^= x >> 33
        x = (x * 0xC4CEB9FE1A85EC53) % 2 ** 64
        return x ^ (x >> 33)
    seen = set()
    for seed in (0, 1, 2 ** 63 + 5):
        for call in range(3):
            for layer in range(3):
                want = fmix64(fmix64(seed + 0x9E3779B97F4A7C15 * (call + 1)) + layer)
                assert mk.layer_seed(seed, call, layer) == want
                seen.add(want)
    assert len(seen) == 27
    s = mk.NeighborSampler([15, 10, -1], seed=4)
    assert s.fanouts == [15, 10, -1] and s.calls == 0 and s.seed == 4
    for bad in ([], [5, 0]):
        with pytest.raises(ValueError, match="fanouts"):
            mk.NeighborSampler(bad)
    with pytest.raises(TypeError, match="CSRGraph"):
        s.sample(object(), torch.zeros(1, dtype=torch.int32))


def test_layers_refuse_what_blocks_do_not_support():
    b = hand_block()
    x = torch.zeros(5, 8)
    supported = 'MaxKSAGEConv and MaxKSAGE with aggregator_type "mean" or "sum"'
    for agg in ("pool", "gcn"):
        with pytest.raises(NotImplementedError, match="does not take a Block") as ei:
            mk.MaxKSAGEConv(8, 8, agg, maxk=4)(b, x)
        assert supported in str(ei.value) and agg in str(ei.value)
    with pytest.raises(NotImplementedError, match="edge_weight") as ei:
        mk.MaxKSAGEConv(8, 8, "mean", maxk=4)(b, x, edge_weight=torch.ones(5))
    assert supported in str(ei.value)
    for layer, name in ((mk.MaxKGCNConv(8, 8, maxk=4), "MaxKGCNConv"),
                        (mk.MaxKGATConv(8, 8, maxk=4), "MaxKGATConv"),
                        (mk.MaxKGINConv(8, maxk=4), "MaxKGINConv")):
        with pytest.raises(NotImplementedError, match=name + " does not take a Block") as ei:
            layer(b, x)
        assert supported in str(ei.value)
    for model, name in ((mk.MaxKGCN(8, 8, 2, 3, maxk=4), "MaxKGCN"),
                        (mk.MaxKGIN(8, 8, 2, 3, maxk=4), "MaxKGIN")):
        with pytest.raises(NotImplementedError, match=name + " does not take a Block"):
            model([b, b], x)
    with pytest.raises(ValueError, match="2 layers, got 1 blocks"):
        mk.MaxKSAGE(8, 8, 2, 3, maxk=4)([b], x)
    # the aggregation's own checks, before any launch
    for bad_x, k, msg in ((torch.zeros(4, 8), 4, "num_src"), (torch.zeros(5, 6), 4, "D % 4"),
                          (torch.zeros(5, 8), 9, "k <= D"), (torch.zeros(5, 260), 4, "<= 256")):
        with pytest.raises(RuntimeError, match=msg):
            mk.block_aggregate(bad_x, b, k)
    with pytest.raises(TypeError, match="Block"):
        mk.block_aggregate(x, mk.CSRGraph(b.ptr, b.idx), 4)
    # a mean layer's parameters are what they were
    torch.manual_seed(1234)
    layer = mk.MaxKSAGEConv(48, 64, "mean")
    assert list(layer.state_dict()) == ["bias", "fc_self.weight", "fc_neigh.weight"]
    assert float(torch.rand(1)) == 0.4580006003379822
