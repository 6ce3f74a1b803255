"""The shared exclusive scan (spgemm-gnn_amd/csrc/scan.h) as the tests of its callers restate it:
tests/sampling.py, tests/subgraph.py and tests/transpose.py name the maxk_scan:: kernels each of
their entry points launches; tests/test_scan_capi.py holds the union to the fixture and to the
library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "spgemm-gnn_amd", "csrc", "scan.h")

WAVE, THREADS, WAVES, ITEMS = 64, 256, 4, 8      # kWave, kThreads, kWaves, kItems
TILE = 2048                                      # kTile: items of a scan tile
ROUND = THREADS                                  # tile sums one round of the partials loop takes
HEADER_CONSTANTS = {"kWave": WAVE, "kThreads": THREADS, "kWaves": WAVES, "kItems": ITEMS,
                    "kTile": TILE}

# what maxk_scan::exclusive_scan launches: the plain scan of an int32 array
PLAIN_KERNELS = ("maxk_scan::apply_kernel", "maxk_scan::partials_kernel<1>",
                 "maxk_scan::tile_sums_kernel<maxk_scan::PlainItem>")

# Scanned lengths at which tiling and the carry can go wrong: one item, one tile - 1 / at / + 1,
# and a full round of the partials loop at / + 1 (the carry into a second round).
LENGTHS = (1, TILE - 1, TILE, TILE + 1, ROUND * TILE, ROUND * TILE + 1)


def tiles(n):
    return (n + TILE - 1) // TILE


def header_constants():
    """The constants above as csrc/scan.h evaluates them."""
    env = {}
    for name, expr in re.findall(r"constexpr int (k\w+) = ([^;]+);", open(HEADER).read()):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))  # noqa: S307 (arithmetic)
    return env
