"""CPU: the inputs of tests/test_gpu_rowconst.py are what their docstrings say, and the numpy
form of the row-constant rule decides the cases the plan has to tell apart."""
import numpy as np

import rowconst as rc
import structured as st


def test_rule_on_small_cases():
    ptr = np.array([0, 0, 1, 4, 6], np.int32)          # rows of 0, 1, 3 and 2 edges
    ok = np.array([7.0, 0.25, 0.25, 0.25, -3.0, -3.0], np.float32)
    assert rc.rowconst_rule(ptr, ok) == 1
    assert rc.rowconst_rule(ptr, None) == 1
    assert rc.rowconst_rule(ptr, np.ones(6, np.float32)) == 1
    for e, x in ((2, 0.5), (5, 3.0), (3, np.nextafter(np.float32(0.25), np.float32(1.0)))):
        v = ok.copy()
        v[e] = x
        assert rc.rowconst_rule(ptr, v) == 0, (e, x)
    # the same bits along a row, but a value the one scaling cannot carry
    for x in (0.0, -0.0, np.nan, np.inf, -np.inf):
        v = ok.copy()
        v[1:4] = x
        assert rc.rowconst_rule(ptr, v) == 0, x
        v = ok.copy()
        v[0] = x                                        # a row of one edge
        assert rc.rowconst_rule(ptr, v) == 0, x
    # +0.0 and -0.0 differ in bits; a denormal constant passes
    v = ok.copy()
    v[1:4] = np.float32(1e-40)
    assert rc.rowconst_rule(ptr, v) == 1
    # no rows, no edges
    assert rc.rowconst_rule(np.zeros(1, np.int32), np.zeros(0, np.float32)) == 1
    assert rc.rowconst_rule(np.zeros(5, np.int32), np.zeros(0, np.float32)) == 1


def test_kernel_forms():
    assert [k for k in (4, 8, 12, 16, 20, 22, 24, 32, 48, 64, 128) if rc.has_rowconst_kernel(k)] \
        == [16, 22, 24, 32, 64, 128]
    assert not rc.has_rowconst_kernel(16, fwd_fixed=False)


def test_graph_shapes():
    p, ix = rc.tiles_graph()
    deg = np.diff(p)
    assert p.size - 1 == 130 and ix.max() < rc.NCOLS and ix.min() >= 0
    assert deg[64:96].sum() == 0 and deg[0] == 0 and deg[1] == 1 and deg[129] == 1
    assert (deg[[10, 40, 41, 100]] >= 2).all()          # the rows the non-finite cases use
    p, ix = rc.heavy_graph()
    deg = np.diff(p)
    assert deg[3] == 9000 and np.unique(ix[p[3]:p[4]]).size < 9000     # repeated columns
    # above the task cap, max(4096, 1.5 x the average tile): the row is split
    tiles = -(-deg.size // rc.TILE)
    assert deg[3] > max(4096, 1.5 * deg.sum() / tiles)


def test_exact_cases_are_exact_and_row_constant():
    for g in rc.GRAPHS:
        for k in (8, 16, 24, 32):
            c = rc.exact_case(g, k)
            assert st.exactly_summable(c.mag) and rc.rowconst_rule(c.p, c.v) == 1
            assert (c.od == np.round(c.od)).all()
    c = rc.exact_case("tiles", 16, dup=True)
    assert (c.oi[::2, 0] == c.oi[::2, 1]).all() and st.exactly_summable(c.mag)
    assert not np.array_equal(c.ref, rc.exact_case("tiles", 16).ref)
    b = rc.exact_case("tiles", 16, break_row=50)
    a = rc.exact_case("tiles", 16)
    assert rc.rowconst_rule(b.p, b.v) == 0 and (a.v != b.v).sum() == 1
    assert st.exactly_summable(b.mag)
    # another seed gives other row values (the refresh test's third step)
    assert (rc.exact_case("tiles", 16, values_seed=2).v != a.v).any()


def test_range_case_mixes_fixed_and_f64_tasks():
    c = rc.range_case()
    assert rc.rowconst_rule(c.p, c.v) == 1
    assert rc.fixed_tasks(c.p, c.od) == [True, False, True]
    a = np.abs(c.od)
    assert a.max() < 2.0 and a.min() >= 2.0 ** -rc.RANGE_E
    assert np.isfinite(c.ref).all()


def test_nonfinite_cases():
    for k in (16, 32):
        for kind, rule in (("val_nan", 0), ("val_inf", 0), ("table", 1)):
            c = rc.nonfinite_case(k, kind)
            assert rc.rowconst_rule(c.p, c.v) == rule
            assert not np.isfinite(c.ref).all()
        c = rc.nonfinite_case(k, "table")
        assert np.isnan(c.ref).any() and (c.ref == np.inf).any() and (c.ref == -np.inf).any()
