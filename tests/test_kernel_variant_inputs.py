"""CPU: the preconditions of tests/test_gpu_kernel_variants.py. Every name of the fixture has a
case; the inputs built in tests/kernel_variants.py are exactly summable; the graphs for grad_out
above 4 GiB have the stated rows; and the restated dispatch agrees with launches worked by hand
from the launcher source (csrc/spgemm.hip, csrc/maxk_topk.hip, csrc/sddmm.hip)."""
import collections

import numpy as np

import kernel_variants as kv
import rowconst
import sweep
from structured import exactly_summable

N = kv.NS


def info(**kw):
    base = dict(dim_k=16, dim_origin=256, num_nodes=600, fwd_layout=4, fwd_fixed=1, fwd_waves=8,
                fwd_unroll=8, fwd_rowconst=0, fwd_split_rows=0, bwd_waves=16, bwd_unroll=8)
    base.update(kw)
    return base


# ------------------------------------------------------------------ the cases and the fixture
def test_every_fixture_name_has_a_case_and_no_case_targets_another_name():
    names = kv.fixture_names()
    targets = collections.Counter(c.target for c in kv.cases())
    assert sorted(set(names) - set(targets)) == []
    assert sorted(set(targets) - set(names)) == []
    assert len(names) == len(set(names))


def test_single_instance_table_is_the_fixture_names_without_a_parameterised_sibling():
    """SINGLES holds exactly the kernels the fixture lists once (by kernel name)."""
    names = kv.fixture_names()
    per_kernel = collections.Counter(n.split("<")[0] for n in names)
    once = {n for n in names if per_kernel[n.split("<")[0]] == 1}
    assert set(kv.SINGLES) == once
    scenarios = {s for s, _, _ in kv.SINGLES.values()}
    assert scenarios <= set(kv.PLAN_SCENARIOS) | {"value_refresh", "stats_odd_k", "topk_count",
                                                  "edge_softmax", "gat_attention"}


def test_families_hold_the_counts_of_the_launchers():
    fam = collections.defaultdict(set)
    for c in kv.cases():
        fam[c.target[len(N):].split("<")[0]].add(c.target)
    assert len(fam["spgemm_fwd_kernel"]) == 27          # 7 x 3 and 3 x 2 with 4-byte words
    assert len(fam["sspmm_bwd4_kernel"]) == 28          # 6 shapes x F x Q and 4 big
    assert len(fam["topk_exact_kernel"]) == 40
    assert len(fam["topk_ref_compat_kernel"]) == 20
    assert len(fam["sspmm_bwd_rows_kernel"]) == 3       # R = 8 is unreachable and not compiled
    assert len(fam["cbsr_stats4_kernel"]) == 5
    assert len(fam["sddmm_edge_grad_kernel"]) == 7
    assert len(fam["dense_spmm_kernel"]) == 5
    assert len(fam["maxk_scatter_backward_kernel"]) == 4
    assert len(fam["pack_cbsr3_kernel"]) == 2


# ------------------------------------------------------------------ exactly summable inputs
def test_plan_cases_are_exactly_summable():
    seen = set()
    for c in kv.cases():
        if "graph" not in c.p:
            continue
        key = (c.p["graph"], c.p["k"])
        if key in seen:
            continue
        seen.add(key)
        if key[0] == "tiles":
            x = rowconst.exact_case("tiles", key[1])
            assert rowconst.rowconst_rule(x.p, x.v) == 1
            assert exactly_summable(x.mag), key
        else:
            x = sweep.case(key[0], 256, key[1])
            assert exactly_summable(x.fwd_mag, x.bwd_mag), key
    for gname, k, _ in kv.PLAN_SCENARIOS.values():
        x = sweep.case(gname, 256, k)
        assert exactly_summable(x.fwd_mag, x.bwd_mag), (gname, k)
    mixed = rowconst.exact_case("tiles", kv.REFRESH_K, break_row=5)
    assert rowconst.rowconst_rule(mixed.p, mixed.v) == 0
    assert exactly_summable(mixed.mag)


def test_row_pass_graphs():
    for r, deg in kv.TP_DEGREES.items():
        c = kv.tp_case(deg)
        assert c.ix.size == kv.TP_ROWS * deg and c.ix.max() < kv.TP_COLS
        assert kv.row_pass_kernel(c.n, c.ix.size) == f"{N}sspmm_bwd_rows_kernel<4, {r}>"
        assert exactly_summable(c.bwd_mag)
        assert np.array_equal(c.bwd, c.bwd.astype(np.float32))


def test_big_graphs_have_the_stated_rows():
    assert kv.BIG_N * 256 * 4 > 2 ** 32 and (kv.BIG_N - 41) * 256 * 4 < 2 ** 32
    rows = kv.BIG_ROWS
    assert np.array_equal(rows, np.unique(rows))
    assert rows[0] == 0 and rows[-1] == kv.BIG_N - 1
    assert {kv.BIG_BOUNDARY - 1, kv.BIG_BOUNDARY} <= set(rows.tolist())
    assert (kv.BIG_BOUNDARY - 1) * 256 * 4 + 255 * 4 < 2 ** 32 <= kv.BIG_BOUNDARY * 256 * 4
    assert sorted(kv.BIG_FQ) == [(2, False), (2, True), (4, False), (4, True)]
    for (f, q), k in kv.BIG_FQ.items():
        c = kv.big_case(k)
        assert (c.deg > 0).all() and 2000 <= c.ix.size <= 5000
        assert c.ix.min() >= 0 and c.ix.max() < kv.BIG_COLS
        ptr = kv.big_ptr(c)
        assert ptr.size == kv.BIG_N + 1 and ptr[-1] == c.ix.size
        assert np.array_equal(np.flatnonzero(np.diff(ptr)), rows)
        assert exactly_summable(c.bwd_mag)
        opts = dict(bwd_algo=1, bwd_features_per_lane=f, bwd_slot_groups=1)
        assert kv.bwd_slots(k, opts, c.n, c.nc, c.ix.size)[:2] == (f, 1)
        name = kv.column_block_kernel(info(num_nodes=c.n, bwd_waves=8, bwd_unroll=8),
                                      *kv.bwd_slots(k, opts, c.n, c.nc, c.ix.size))
        assert name == f"{N}sspmm_bwd4_kernel<8, 512, {f}, {'true' if q else 'false'}, true>"


def test_dense_spmm_and_attention_inputs_are_exact():
    for d in kv.DENSE_SPMM_DS:
        x, y, mag = kv.dense_spmm_case(d)
        assert exactly_summable(mag) and np.array_equal(y, y.astype(np.float32))
    c = kv.attention_case()
    assert c.idx.min() >= 0 and c.idx.max() < c.nc
    lengths = np.diff(c.ptr)
    assert all(n == 0 or n & (n - 1) == 0 for n in lengths.tolist())
    # the score is constant along every row, and both leaky branches occur
    for r in range(c.n):
        z = c.z[c.ptr[r]:c.ptr[r + 1]]
        assert z.size == 0 or (z == z[0]).all()
    assert (c.z > 0).any() and (c.z < 0).any()
    # 1 / length and every gradient are f32 numbers, and their sums too
    assert np.array_equal(c.alpha.astype(np.float64), 1.0 / np.repeat(lengths, lengths))
    for ref in kv.attention_refs(c):
        assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------ hand-worked launches
def test_forward_dispatch_by_hand():
    # k = 16 default: pair chunks (FL 4), fixed point, 8 lanes per edge: quads (FL 6), 8 waves
    assert kv.forward_kernel(info()) == N + "spgemm_fwd_kernel<4, 6, 512, 8, false>"
    # the issue's example: packed records, f64, 8 waves, 4 sub-steps
    assert kv.forward_kernel(info(fwd_layout=1, fwd_fixed=0, fwd_unroll=4)) == \
        N + "spgemm_fwd_kernel<4, 0, 512, 4, false>"
    # k = 24 lane chunks: 8 lanes, fixed: FL 1 | 2; row-constant values, 4 waves
    assert kv.forward_kernel(info(dim_k=24, fwd_layout=2, fwd_waves=4, fwd_rowconst=1)) == \
        N + "spgemm_fwd_kernel<4, 3, 256, 8, true>"
    # k = 20 lane chunks: 7 lanes, no quads
    assert kv.forward_kernel(info(dim_k=20, fwd_layout=2)) == \
        N + "spgemm_fwd_kernel<4, 1, 512, 8, false>"
    # k = 8 two tables with fixed point asked: 2 lanes, no quads
    assert kv.forward_kernel(info(dim_k=8, fwd_layout=0, fwd_waves=4)) == \
        N + "spgemm_fwd_kernel<4, 0, 256, 8, false>"
    # k = 201: one feature per lane
    assert kv.forward_kernel(info(dim_k=201, fwd_layout=3, fwd_fixed=0)) == \
        N + "spgemm_fwd_kernel<1, 0, 512, 8, false>"
    # 4 waves never run 4 sub-steps (check_options refuses the pair; the launcher ignores it)
    assert kv.forward_kernel(info(fwd_waves=4, fwd_unroll=4)).endswith("<4, 6, 256, 8, false>")


def test_forward_pass_dispatch_by_hand():
    s4, z, p3 = N + "cbsr_stats4_kernel", N + "zero_rows_kernel", N + "pack_cbsr3_kernel"
    assert kv.forward_pass_kernels(info()) == [s4 + "<2, true>"]
    assert kv.forward_pass_kernels(info(fwd_fixed=0)) == [s4 + "<2, false>"]
    assert kv.forward_pass_kernels(info(fwd_layout=1)) == [s4 + "<1, true>"]
    assert kv.forward_pass_kernels(info(fwd_layout=0)) == [s4 + "<0, true>"]
    assert kv.forward_pass_kernels(info(fwd_layout=0, fwd_fixed=0, fwd_split_rows=1)) == [z]
    assert kv.forward_pass_kernels(info(fwd_layout=0), stats_given=True) == []
    assert kv.forward_pass_kernels(info(dim_k=24, fwd_layout=2, fwd_split_rows=1)) == \
        [p3 + "<3>", s4 + "<0, true>"]
    assert kv.forward_pass_kernels(info(dim_k=18, fwd_layout=4, fwd_split_rows=1)) == \
        [p3 + "<2>", z, N + "cbsr_stats_kernel"]
    assert kv.forward_pass_kernels(info(dim_k=5, fwd_layout=3, fwd_fixed=0, fwd_split_rows=2)) == [z]


def test_backward_dispatch_by_hand():
    e = sweep.edges("sparse")
    # the sparse graph at k = 16: two slot groups of 8 slots, so two slots per lane, 4 lanes
    assert kv.bwd_slots(16, {}, 600, 600, e) == (2, 2, 16)
    assert kv.column_block_kernel(info(), 2, 2, 16) == N + "sspmm_bwd4_kernel<8, 1024, 2, true, false>"
    # k = 10: F = 2 (k % 4 == 2), 5 lanes; asked F = 4: padded to 12, 3 lanes
    assert kv.bwd_slots(10, {}, 600, 600, e) == (2, 1, 10)
    assert kv.bwd_slots(10, dict(bwd_features_per_lane=4), 600, 600, e) == (4, 1, 12)
    # k = 200 with two slots asked: 100 lanes exceed a wave, runs 4
    assert kv.bwd_slots(200, dict(bwd_features_per_lane=2), 600, 600, e)[0] == 4
    # 4 slot groups at k = 24, F = 4: 4 x 4 does not divide 24, halved to 2
    assert kv.bwd_slots(24, dict(bwd_slot_groups=4, bwd_features_per_lane=4), 600, 600, e) == (4, 2, 24)
    for (w, u), shape in {(16, 8): "8, 1024", (12, 12): "12, 768", (12, 8): "8, 768",
                          (8, 16): "16, 512", (8, 12): "12, 512", (8, 8): "8, 512"}.items():
        assert kv.column_block_kernel(info(bwd_waves=w, bwd_unroll=u), 4, 1, 12) == \
            f"{N}sspmm_bwd4_kernel<{shape}, 4, false, false>"
    assert kv.row_pass_kernel(600, 600 * 256) == N + "sspmm_bwd_rows_kernel<4, 1>"
    assert kv.row_pass_kernel(600, 600 * 255) == N + "sspmm_bwd_rows_kernel<4, 2>"
    assert kv.row_pass_kernel(600, 600 * 3) == N + "sspmm_bwd_rows_kernel<4, 4>"


def test_topk_and_scatter_dispatch_by_hand():
    t, r = N + "topk_exact_kernel", N + "topk_ref_compat_kernel"
    assert kv.topk_kernel("exact", 40, 256, 16) == t + "<4, false, true, false, false, false, false>"
    assert kv.topk_kernel("exact", 1 << 20, 256, 16) == \
        t + "<8, false, true, false, false, false, false>"
    assert kv.topk_kernel("exact", 1 << 20, 256, 65).startswith(t + "<4, true, true")
    assert kv.topk_kernel("exact", 1 << 20, 200, 16, stats=True).startswith(t + "<4, false, false, true")
    # dropout without a record still runs a record kernel
    assert kv.topk_kernel("exact", 40, 200, 72, dropout=True) == \
        t + "<4, true, false, false, true, true, false>"
    # dense, partial row, statistics, k <= 64: the k > 64 kernel
    assert kv.topk_kernel("exact", 40, 200, 16, stats=True, dense=True) == \
        t + "<4, true, false, true, true, false, true>"
    assert kv.topk_kernel("exact", 40, 200, 16, dense=True, dropout=True) == \
        t + "<4, false, false, false, true, true, true>"
    assert kv.topk_kernel("ref_compat", 40, 256, 16, stats=True, records=True) == \
        r + "<true, true, true, false, false>"
    assert kv.topk_kernel("ref_compat", 40, 200, 16, dense=True) == \
        r + "<false, false, true, false, true>"
    assert kv.scatter_kernel(True, False) == N + "maxk_scatter_backward_kernel<true, false>"
    assert [kv.sddmm_kernel(k)[-4:] for k in (1, 4, 5, 8, 9, 129)] == \
        ["l<1>", "l<1>", "l<2>", "l<2>", "l<4>", "<64>"]
    assert [kv.dense_spmm_kernel(d) for d in (4, 16, 20, 132)] == \
        [N + "dense_spmm_kernel<4, 4>", N + "dense_spmm_kernel<4, 4>",
         N + "dense_spmm_kernel<8, 4>", N + "dense_spmm_kernel<64, 4>"]
