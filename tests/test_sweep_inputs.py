"""CPU: the preconditions of the k / D sweep (tests/sweep.py), which let tests/test_gpu_sweep.py
demand equality: every case is exactly summable on the oracle's magnitudes, the two graphs have
the density classes, empty rows and split rows the sweep relies on, and the expectation table
covers every case exactly once."""
import collections

import numpy as np
import pytest

import structured as st
import sweep
from oracle import oracle


# ---------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
@pytest.mark.parametrize("gname", ["sparse", "dense"])
def test_plan_and_autograd_cases_are_exactly_summable(gname, lo, hi):
    """Every (graph, D = 256, k, p) of the plan, SDDMM and autograd sections: the forward's,
    the backward's and x.grad's sums of |terms| stay within 2^22, also with the dense output's
    integer gradient (|g| <= 4) merged in before the dropout scale."""
    for k in range(lo, hi + 1):
        for p in (0.0, sweep.DROP_P):
            c = sweep.case(gname, sweep.D_FULL, k, p)
            assert st.exactly_summable(c.fwd_mag, c.bwd_mag, c.gx_mag), (gname, k, p)
            assert st.exactly_summable((c.bwd_mag.astype(np.float64) + 4.0) * 2.0)
            # integers times {0.5, 1, 2} (times 2): every term is a multiple of 0.5
            assert np.array_equal(c.od * 2, np.round(c.od * 2))
        # SDDMM: k products of two integers in [-4, 4] (times the dropout scale)
        assert k * 4.0 * 4.0 * 2.0 <= st.EXACT_LIMIT


@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_d_sweep_cases_are_exactly_summable(lo, hi):
    for d in range(lo, hi + 1):
        for k in sweep.d_sweep_ks(d):
            c = sweep.case("sparse", d, k)
            assert st.exactly_summable(c.fwd_mag, c.bwd_mag), (d, k)


def test_d_sweep_ks():
    assert sweep.d_sweep_ks(1) == [1] and sweep.d_sweep_ks(2) == [1, 2]
    assert sweep.d_sweep_ks(5) == [1, 3, 5] and sweep.d_sweep_ks(256) == [1, 128, 256]


# ---------------------------------------------------------------------------- graphs
@pytest.mark.parametrize("gname", ["sparse", "dense"])
def test_graph_structure(gname):
    p, ix, v = sweep.graph(gname)
    assert p.dtype == np.int32 and ix.dtype == np.int32 and v.dtype == np.float32
    assert p.size == sweep.N + 1 and p[0] == 0 and p[-1] == ix.size == v.size
    deg = np.diff(p)
    assert (deg >= 0).all() and ix.min() >= 0 and ix.max() < sweep.N
    for r in range(sweep.N):                           # columns sorted within each row
        assert (np.diff(ix[p[r]:p[r + 1]]) >= 0).all(), r
    assert set(np.unique(v)) == {0.5, 1.0, 2.0}
    for r in sweep.EMPTY_ROWS[gname]:                  # first and last row among them
        assert deg[r] == 0
    assert (deg == 0).sum() >= len(sweep.EMPTY_ROWS[gname])
    h = sweep.HEAVY_ROW[gname]
    assert deg[h] == sweep.HEAVY_EDGES[gname] and deg[h] == deg.max()
    assert np.sort(deg)[-2] <= 64                      # no other row is near a task cap
    again = sweep.graph.__wrapped__(gname)             # deterministic
    assert all(np.array_equal(a, b) for a, b in zip(again, (p, ix, v)))


def test_density_classes():
    """sparse: about 3 edges per row, below both thresholds at every k they are asked at;
    dense: about 23 per row beside the heavy row, above both. Neither reaches the automatic
    two-pass backward (below 0.75 edges per block row), so bwd_algo 3 runs by option."""
    assert 2.5 <= sweep.edges("sparse") / sweep.N <= 3.5
    rest = sweep.edges("dense") - sweep.HEAVY_EDGES["dense"]
    assert 22.0 <= rest / sweep.N <= 26.0
    assert sweep.edges_per_block_row("sparse", 8) < 10.0
    assert sweep.edges_per_block_row("dense", 8) >= 10.0
    for k in range(16, 257, 8):
        assert sweep.edges_per_block_row("sparse", k) < 4.5, k
        assert sweep.edges_per_block_row("dense", k) >= 4.5, k
    for g in ("sparse", "dense"):
        for k in sweep.K_ALL:
            assert not sweep.expected(g, k, {}).twopass, (g, k)


def test_split_rows():
    """dense: the heavy row is several times the forward's default cap (max(4096, 1.5 x the
    average 32-row tile)); sparse: several times the cap of the fwd_task_cap option set, and
    below the default cap, which 600 unique columns cannot reach."""
    tiles = -(-sweep.N // 32)
    for g in ("sparse", "dense"):
        avg = -(-sweep.edges(g) // tiles)
        assert avg + avg // 2 <= sweep.FWD_MIN_TASK_CAP
    assert sweep.HEAVY_EDGES["dense"] >= 3 * sweep.FWD_MIN_TASK_CAP
    assert sweep.N < sweep.FWD_MIN_TASK_CAP
    assert sweep.HEAVY_EDGES["sparse"] >= 5 * sweep.SPARSE_TASK_CAP
    assert sweep.expected("dense", 16, {}).info["fwd_split_rows"] == 1
    assert sweep.expected("sparse", 16, {}).info["fwd_split_rows"] == 0
    assert sweep.expected("sparse", 16, dict(fwd_task_cap=64)).info["fwd_split_rows"] == 1


def test_dense_graph_has_a_hub_column():
    p, ix, _ = sweep.graph("dense")
    indeg = st.col_degrees(p, ix)
    rows_with = np.unique(np.repeat(np.arange(sweep.N), np.diff(p))[ix == sweep.HUB_COL])
    assert rows_with.size == (np.diff(p) > 0).sum()                # every non-empty row
    assert indeg[sweep.HUB_COL] == indeg.max() >= 5 * np.median(indeg)
    # a column block of the backward spans several rows: every block holds >= 100 columns
    assert min(sweep.expected("dense", k, {}).info["bwd_block_cols"] for k in sweep.K_ALL) >= 100


# ---------------------------------------------------------------------------- the table
def test_table_covers_every_case_exactly_once():
    cases = sweep.all_cases()
    assert len(cases) == len(set(cases)), [c for c, n in collections.Counter(cases).items()
                                           if n > 1][:5]
    t = sweep.table()
    with_expectation = [c for c in cases if c[0] in ("plan", "records")]
    assert set(t) == set(with_expectation) and len(t) == len(with_expectation)
    assert len(with_expectation) == 256 * (2 + len(sweep.OPTION_SETS)) + 256 * 3
    assert len(sweep.OPTIONS) == len(sweep.OPTION_SETS) + 1       # distinct ids


def test_number_of_refusals():
    t = sweep.table()
    refused = [c for c, e in t.items()
               if (e if c[0] == "records" else (e.code if e.kind == "refused" else 0)) != 0]
    assert len(refused) == sweep.EXPECTED_REFUSALS == 448
    assert all(c[0] == "records" and t[c] == sweep.INVALID for c in refused)
    by_layout = collections.Counter(c[2] for c in refused)
    assert by_layout == {1: 192, 2: 64, 4: 192}


def test_table_pins():
    """Rows of the table the header's text names outright."""
    ex = sweep.expected
    i16 = ex("sparse", 16, {})
    assert (i16.info["fwd_layout"], i16.info["fwd_waves"], i16.F, i16.S) == (4, 8, 2, 2)
    assert ex("dense", 16, {}).S == 1 and ex("dense", 16, {}).F == 4
    assert ex("sparse", 8, {}).F == 2 and ex("dense", 8, {}).F == 4
    assert ex("sparse", 48, {}).info["fwd_unroll"] == 4
    assert ex("sparse", 48, dict(fwd_waves=4)).info["fwd_unroll"] == 8
    assert ex("sparse", 16, dict(fwd_chunk3=2)).info["fwd_waves"] == 4
    assert ex("sparse", 126, {}).F == 2 and ex("sparse", 130, {}).F == 4
    assert ex("sparse", 130, dict(bwd_features_per_lane=2)).kind == "fallback"
    assert ex("sparse", 128, dict(bwd_features_per_lane=2)).F == 2
    assert [ex("sparse", k, {}).info["fwd_layout"] for k in (190, 191, 192, 193, 194, 196)] == \
        [2, 2, 0, 3, 3, 0]
    assert ex("sparse", 193, dict(fwd_fixed=1)).info["fwd_fixed"] == 0
    assert ex("sparse", 12, dict(fwd_fixed=1)).info["fwd_fixed"] == 1
    assert ex("sparse", 15, {}).info["fwd_fixed"] == 0
    assert ex("sparse", 17, {}).info["fwd_fixed"] == 1
    assert ex("sparse", 64, dict(fwd_two_tables=2)).info["fwd_layout"] == 1
    assert ex("sparse", 130, dict(fwd_chunk3=3)).info["fwd_layout"] == 2
    assert ex("sparse", 128, dict(fwd_chunk3=3)).info["fwd_layout"] == 4
    tp = [k for k in sweep.K_ALL if ex("sparse", k, dict(bwd_algo=3)).twopass]
    assert tp == [4, 8, 16, 32, 64, 128, 256]
    assert ex("sparse", 24, dict(bwd_algo=3)).kind == "fallback"
    assert ex("sparse", 24, dict(bwd_slot_groups=4)).S == 2          # 24 = 4 x 2 x 3
    assert ex("sparse", 32, dict(bwd_slot_groups=4)).S == 4
    assert ex("sparse", 10, dict(bwd_waves=8)).info["bwd_unroll"] == 12
    assert ex("sparse", 12, dict(bwd_waves=8)).info["bwd_unroll"] == 8
    assert ex("sparse", 10, {}).info["bwd_waves"] == 16
    assert ex("sparse", 10, {}).info["bwd_unroll"] == 8


# ---------------------------------------------------------------------------- top-k rows
@pytest.mark.parametrize("d", sweep.D_LIST)
def test_topk_rows(d):
    x = sweep.topk_rows(d)
    assert x.shape == (40, d) and x.dtype == np.float32
    assert np.isfinite(x[:sweep.TOPK_FINITE]).all()
    assert np.isnan(x[38]).all() and np.signbit(x[38]).all()
    assert len(set(x[28])) == 1
    assert np.isnan(x[37]).any() and np.isnan(x[39]).any() == (d >= 2)
    if d >= 12:
        assert np.isinf(x[36]).sum() == 2
    if d >= 2:
        assert np.signbit(x[29]).any() and not np.signbit(x[29]).all() and (x[29] == 0).all()


@pytest.mark.parametrize("d,k", [(256, 1), (256, 16), (256, 100), (256, 256), (65, 33), (5, 3),
                                 (1, 1)])
def test_ref_compat_counts_against_the_oracle(d, k):
    """The count restatement reproduces the oracle's ref_compat table: the first `count` entries
    above p in index order, then (0.0f, 0) padding. Checked through what the table shows: slots
    at and past `count` are padding, and the slots before it hold ascending selectors."""
    x = sweep.topk_rows(d)
    od, oi = oracle.maxk(x, k, "ref_compat")
    cnt = sweep.ref_compat_counts(x, k)
    assert cnt.shape == (40,) and (cnt >= 0).all() and (cnt <= k).all()
    assert (cnt[:26] > 0).all() or d == 1              # N(0, 1) rows select something
    for r in range(40):
        c = int(cnt[r])
        assert (od[r, c:].view(np.uint32) == 0).all() and (oi[r, c:] == 0).all(), (r, c)
        assert (np.diff(oi[r, :c].astype(int)) > 0).all(), r
        if c:                                          # the last filled slot is not padding
            assert oi[r, c - 1] != 0 or c == 1
            assert od[r, c - 1] == x[r, oi[r, c - 1]]
    assert cnt[28] == 0 and cnt[30] == 0               # constant rows fill nothing
    assert (sweep.topk_counts(x, k, "exact") == k).all()
