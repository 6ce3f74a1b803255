"""Shared by tests/test_sampling_capi.py (CPU) and tests/test_gpu_sampling.py (GPU): numpy
restatements of the neighbour sampler and the block compaction of include/maxk_hip.h ("Neighbour
sampling"), the test graphs and seed sets, and float64 restatements of the block aggregation and
of the SAGE layer on blocks.

The sampler's rule is part of the ABI, so everything here is exact: the hash, the ranks, the kept
set, the order of the output and the relabelling are compared bit for bit."""
import functools

import numpy as np

import gat_heads as gh
import scan
from gat_heads import NUM, bound, exact_grad, rows_of  # noqa: F401  (used by the test modules)

LIMITS = (16, 512)               # maxk_sample_row_limits, asserted against the library
FANOUTS = (1, 2, 10, 25, 64)     # and one above the longest row, and -1 (every neighbour)
M32 = np.uint64(0xFFFFFFFF)
KERNELS = ("maxk_sp::compact_init_kernel", "maxk_sp::compact_mark_kernel",
           "maxk_sp::compact_place_kernel", "maxk_sp::compact_relabel_kernel",
           "maxk_sp::sample_count_kernel")
# the maxk_scan:: kernels of the compaction: its tile sums count new and seed columns
COMPACT_SCAN_KERNELS = ("maxk_scan::partials_kernel<2>",
                        "maxk_scan::tile_sums_kernel<maxk_sp::ColumnItem>")
SCAN_KERNELS = scan.PLAIN_KERNELS + COMPACT_SCAN_KERNELS     # every maxk_scan:: name restated here
SAMPLER_KERNELS = KERNELS[4:] + scan.PLAIN_KERNELS
COMPACT_KERNELS = KERNELS[:4] + COMPACT_SCAN_KERNELS
SCAN_TILE = scan.TILE            # items of a scan tile (csrc/scan.h)


def sample_kernel_name(fanout):
    return f"maxk_sp::sample_kernel<{'true' if fanout < 0 else 'false'}>"


def regime(n):
    return 0 if n <= LIMITS[0] else 1 if n <= LIMITS[1] else 2


def sample_scratch_bytes(num_seeds):
    return 4 * (2 * ((num_seeds + 1 + SCAN_TILE - 1) // SCAN_TILE) + 2)


def compact_scratch_bytes(num_cols):
    return 4 * (num_cols + 2 * ((num_cols + SCAN_TILE - 1) // SCAN_TILE) + 2)


# ------------------------------------------------------------------ the hash and the selection
def fmix32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def edge_key(seed, e):
    """key(e): uint64 array holding the 32-bit keys of the edge numbers e under the 64-bit seed."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    e = np.asarray(e, np.uint64) & M32
    return fmix32(fmix32(e ^ lo) ^ fmix32(((e * np.uint64(0x9E3779B1)) & M32) + hi))


def edge_rank(seed, e):
    return (edge_key(seed, e) << np.uint64(32)) | (np.asarray(e, np.uint64) & M32)


def kept_edges(b, n, fanout, seed):
    """Edge numbers kept of the row [b, b + n), ascending."""
    e = np.arange(b, b + n, dtype=np.int64)
    if fanout < 0 or n <= fanout:
        return e
    order = np.argsort(edge_rank(seed, e), kind="stable")
    return np.sort(e[order[:fanout]])


def sample_ref(ptr, idx, seeds, fanout, seed):
    """(out_ptr int32 [S + 1], out_col int32, out_eid int32) of maxk_sample_neighbors."""
    eids = [kept_edges(int(ptr[r]), int(ptr[r + 1] - ptr[r]), fanout, seed) for r in seeds]
    out_ptr = np.zeros(len(eids) + 1, np.int64)
    np.cumsum([len(x) for x in eids], out=out_ptr[1:])
    eid = np.concatenate(eids).astype(np.int64) if eids else np.zeros(0, np.int64)
    return out_ptr.astype(np.int32), idx[eid].astype(np.int32), eid.astype(np.int32)


def compact_ref(seeds, cols, num_cols):
    """(src_ids int32 [num_src], local_col int32, (num_src, distinct_seeds)) of
    maxk_block_compact: the seeds in the given order, then every other sampled column once,
    ascending; a repeated seed column maps to its lowest position."""
    seeds, cols = np.asarray(seeds, np.int64), np.asarray(cols, np.int64)
    mark = np.full(num_cols, -1, np.int64)
    for i in range(seeds.size - 1, -1, -1):       # the lowest position wins
        mark[seeds[i]] = i
    new = np.setdiff1d(np.unique(cols), seeds)
    mark[new] = seeds.size + np.arange(new.size)
    src = np.concatenate([seeds, new]).astype(np.int32)
    return src, mark[cols].astype(np.int32), (int(src.size), int(np.unique(seeds).size))


# ------------------------------------------------------------------ graphs and seed sets
def square_graph():
    """The 600 x 600 graph of the multi-head tests (hub row 5,000, hub column 3,000)."""
    return gh.graph_arrays() + (NUM,)


RECT_ROWS, RECT_COLS = 300, 900
RECT_DESIGNED = (0, 1, 2, 3, 9, 10, 11, 24, 25, 26, 63, 64, 65, LIMITS[0] - 1, LIMITS[0],
                 LIMITS[0] + 1, LIMITS[1] - 1, LIMITS[1], LIMITS[1] + 1, 2000)


@functools.lru_cache(maxsize=None)
def rect_graph():
    """(ptr, idx, num_cols): 300 rows over 900 columns; the first rows have the designed lengths
    (f - 1, f, f + 1 of every fanout, every limit - 1 / at / + 1, a hub of 2,000), the rest are
    random and short. Columns are ascending within a row and may repeat in the long rows."""
    rng = np.random.default_rng(17)
    deg = np.concatenate([RECT_DESIGNED,
                          rng.integers(0, 40, RECT_ROWS - len(RECT_DESIGNED))]).astype(np.int64)
    rows = np.repeat(np.arange(RECT_ROWS), deg)
    cols = rng.integers(0, RECT_COLS, rows.size)
    order = np.lexsort((cols, rows))
    ptr = np.zeros(RECT_ROWS + 1, np.int64)
    np.cumsum(deg, out=ptr[1:])
    ptr, idx = ptr.astype(np.int32), cols[order].astype(np.int32)
    for a in (ptr, idx):
        a.setflags(write=False)
    return ptr, idx, RECT_COLS


GRAPHS = {"square": square_graph, "rect": rect_graph}


def hub_row(ptr):
    return int(np.argmax(np.diff(ptr)))


def empty_row(ptr):
    return int(np.argmin(np.diff(ptr)))


def seed_sets(ptr):
    """name -> int32 seeds: all rows, a permutation, the hub row, an empty row, none."""
    n = ptr.size - 1
    return {"all": np.arange(n, dtype=np.int32),
            "permutation": np.random.default_rng(3).permutation(n).astype(np.int32),
            "hub": np.array([hub_row(ptr)], np.int32),
            "empty_row": np.array([empty_row(ptr)], np.int32),
            "none": np.zeros(0, np.int32)}


def fanouts_for(ptr):
    return FANOUTS + (int(np.diff(ptr).max()) + 1, -1)


@functools.lru_cache(maxsize=None)
def tie_break_case():
    """(seed, fanout, e0, e1): a 64-bit seed under which two edges e0 < e1 of the square graph's
    hub row share their 32-bit key, and the fanout at which the threshold falls between them: e0
    is the last edge kept and e1 the first one dropped, so only the edge number decides. Found
    by search (about 5,000^2 / 2^33 pairs per seed collide)."""
    ptr, _, _ = square_graph()
    r = hub_row(ptr)
    e = np.arange(ptr[r], ptr[r + 1], dtype=np.int64)
    for seed in range(1, 20000):
        key = edge_key(seed, e)
        order = np.argsort(key, kind="stable")
        same = np.nonzero(key[order][1:] == key[order][:-1])[0]
        if same.size:
            at = int(same[0])
            rank_order = np.argsort(edge_rank(seed, e), kind="stable")
            e0, e1 = int(e[rank_order[at]]), int(e[rank_order[at + 1]])
            assert e0 < e1 and key[rank_order[at]] == key[rank_order[at + 1]]
            return seed, at + 1, e0, e1
    raise AssertionError("no seed with a key collision in the hub row")


# ------------------------------------------------------------------ blocks, float64
def block_ref(ptr, idx, num_cols, seeds, fanout, seed):
    """The block of one layer as numpy arrays: dict(ptr, col (local), eid, src_ids, num_dst,
    num_src)."""
    out_ptr, col, eid = sample_ref(ptr, idx, seeds, fanout, seed)
    src, local, (num_src, distinct) = compact_ref(seeds, col, num_cols)
    assert distinct == len(seeds)
    return dict(ptr=out_ptr, col=local, eid=eid, src_ids=src, num_dst=len(seeds),
                num_src=num_src)


def block_values(bptr, kind):
    deg = np.diff(bptr).astype(np.float64)
    if kind == "sum":
        return np.ones(int(bptr[-1]), np.float32)
    return np.repeat((np.float32(1.0) / np.maximum(deg, 1).astype(np.float32)),
                     np.diff(bptr)).astype(np.float32)


def dense_block(bptr, bcol, val, num_src):
    """A_block as a float64 [num_dst, num_src] matrix (repeated pairs add)."""
    a = np.zeros((bptr.size - 1, num_src))
    np.add.at(a, (rows_of(bptr), bcol), val.astype(np.float64))
    return a


def maxk_dense64(x, k):
    """densify(MaxK(x, k)) in float64: the k largest of each row, ties to the lower index."""
    x = np.asarray(x)
    order = np.argsort(-x.astype(np.float64), axis=1, kind="stable")[:, :k]
    out = np.zeros(x.shape)
    rows = np.arange(x.shape[0])[:, None]
    out[rows, order] = x[rows, order]
    mask = np.zeros(x.shape, bool)
    mask[rows, order] = True
    return out, mask


def exact_features(n, D, seed):
    """Multiples of 0.5 in [-4, 4] with distinct magnitudes per row broken by index: every sum
    of a few thousand of them times a power of two is exact in f32."""
    return (np.random.default_rng(seed).integers(-8, 9, (n, D)) * 0.5).astype(np.float32)
