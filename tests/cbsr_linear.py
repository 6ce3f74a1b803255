"""Cases, inputs and float64 restatements of the CBSR-times-table products (include/maxk_hip.h,
"MaxK linear layers"), shared by tests/test_cbsr_linear_capi.py and tests/test_gpu_cbsr_linear.py.
Every restatement returns, next to its result, the sum of the absolute terms of each element."""
import numpy as np

U = 2.0 ** -24
QUANTUM = 2.0 ** -6          # products of two multiples of 1/8
WAVES, GROUPS = 16, 256      # kLinWaves, kLinGroups of csrc/variants_linear.h
MATMUL, SAMPLED, WEIGHT_GRAD = 0, 1, 2

# (N, D, k, M): N around the wave (64) and the row block (16 rows) up to several work-groups, M on
# both sides of a panel edge of either width and of a lane's columns, k up to D, past one round of
# 64 slots and off the slot tile of 16. The last walks more row blocks than it has work-groups.
CASES = [(1, 16, 1, 1), (63, 16, 16, 4), (65, 100, 8, 63), (257, 100, 32, 64),
         (1000, 256, 16, 65), (65, 256, 256, 127), (257, 100, 100, 128), (257, 256, 64, 129),
         (63, 256, 8, 256), (1000, 256, 16, 260), (1000, 16, 8, 644)]


def panel(d, m):
    mp = 128 if m > 64 else 64
    return mp, -(-m // mp)


def row_groups(n, panels):
    return max(1, min(-(-n // WAVES), 1 if panels >= GROUPS else GROUPS // panels))


def scratch_bytes(op, n, d, k, m):
    if n < 0 or not 1 <= k <= d <= 256 or m < 1 or op not in (0, 1, 2):
        return -1
    mp, p = panel(d, m)
    w = row_groups(n, p)
    return (0, 4 * p * n * k if p > 1 else 0, 4 * (p * w * d * mp + w * d))[op]


def kernels(d, m):
    mp, p = panel(d, m)
    names = {f"maxk_lin::cbsr_{n}_kernel<{mp}>" for n in ("matmul", "sampled", "weight_grad")}
    return names | {"maxk_lin::cbsr_weight_reduce_kernel"} | \
        ({"maxk_lin::cbsr_sampled_sum_kernel"} if p > 1 else set())


def inputs(n, d, k, m, seed, exact, repeat=False):
    """(v [n, k], s [n, k] u8, T [d, m], g [n, m], bias [m]) in f32: standard normal, or for
    `exact` multiples of 1/8 in [-1, 1]. Selectors are distinct within a row and unsorted;
    `repeat` copies the row's first selector into every odd slot."""
    rng = np.random.default_rng(seed)
    def draw(*shape):
        if exact:
            return (rng.integers(-8, 9, shape) / 8).astype(np.float32)
        return rng.standard_normal(shape).astype(np.float32)
    s = np.argsort(rng.random((n, d)), axis=1)[:, :k].astype(np.uint8)
    if repeat:
        s[:, 1::2] = s[:, :1]
    return draw(n, k), s, draw(d, m), draw(n, m), draw(m)


def densify64(v, s, d):
    out = np.zeros((v.shape[0], d))
    np.add.at(out, (np.arange(v.shape[0])[:, None], s.astype(np.int64)), v.astype(np.float64))
    return out


def matmul64(v, s, T, bias=None):
    T = T.astype(np.float64)
    b = 0.0 if bias is None else bias.astype(np.float64)
    d = T.shape[0]
    return densify64(v, s, d) @ T + b, densify64(np.abs(v), s, d) @ np.abs(T) + np.abs(b)


def sampled64(g, s, T):
    g, T, rows = g.astype(np.float64), T.astype(np.float64), np.arange(g.shape[0])[:, None]
    return (g @ T.T)[rows, s.astype(np.int64)], (np.abs(g) @ np.abs(T).T)[rows, s.astype(np.int64)]


def weight_grad64(v, s, g, d):
    """(dT, dsum, sum |terms| of dT, of dsum, count [d] of the (row, slot) pairs per feature)."""
    g = g.astype(np.float64)
    dense, mag = densify64(v, s, d), densify64(np.abs(v), s, d)
    return (dense.T @ g, dense.sum(0), mag.T @ np.abs(g), mag.sum(0),
            np.bincount(s.reshape(-1), minlength=d))


def worst(got, want, mag, terms):
    """The largest error of `got` in units of its bound (terms + 2) u sum |terms|; an element
    without terms must be exactly zero."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    bound = (np.asarray(terms, np.float64) + 2) * U * mag
    err = np.abs(got - want)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
