"""CPU: the shared pieces of the graph operators. The maxk_scan:: kernels (csrc/scan.h) that
tests/sampling.py, tests/subgraph.py and tests/transpose.py restate are together the fixture
tests/golden/kernel_instantiations_scan.txt, which is the library's set, so the closing coverage
tests of the three GPU modules cover every compiled scan kernel between them; the restated
constants are the header's; and the one argument check (maxk::check_ranges, csrc/common.h) refuses
the same four mistakes with the same code and text through one entry point of each file that
calls it (made-up device pointers: nothing reaches a GPU)."""
import ctypes
import os
import sys

import pytest

import sampling as sp
import scan
import subgraph as sg
import transpose as tr
from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instantiations_scan.txt")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_list  # noqa: E402

P = ctypes.c_void_p
lib = _lib.lib
INVALID = -1


# ------------------------------------------------------------------ names, constants
def test_the_three_modules_restate_the_fixture_between_them():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names)) and all(n.startswith("maxk_scan::") for n in names)
    restated = set(sp.SCAN_KERNELS) | set(sg.SCAN_KERNELS) | set(tr.SCAN_KERNELS)
    assert restated == set(names) and len(names) == 7
    # the plain scan is shared; the fused tile sums and their middle steps have one caller each
    assert set(scan.PLAIN_KERNELS) == set(tr.SCAN_KERNELS) <= set(sp.SAMPLER_KERNELS)
    assert set(sp.COMPACT_SCAN_KERNELS) <= set(sp.COMPACT_KERNELS)
    assert set(sg.SCAN_KERNELS) <= set(sg.COUNT_KERNELS)
    assert not set(sg.FILL_KERNELS) & set(names)


def test_fixture_equals_the_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("llvm-readelf not found")
    assert kernel_list.compiled(_lib.LIB_PATH, prefix="maxk_scan::") == \
        kernel_list.read_list(FIXTURE)
    assert kernel_list.main([_lib.LIB_PATH, "--namespace", "maxk_scan::", "--diff", FIXTURE]) == 0


def test_restated_constants_are_the_headers():
    got = scan.header_constants()
    for name, want in scan.HEADER_CONSTANTS.items():
        assert got[name] == want, (name, got[name], want)
    assert scan.TILE == scan.THREADS * scan.ITEMS and scan.WAVES * scan.WAVE == scan.THREADS
    assert sp.SCAN_TILE == sg.SCAN_TILE == tr.SCAN_TILE == scan.TILE
    assert scan.LENGTHS == (1, 2047, 2048, 2049, 524288, 524289)
    assert [scan.tiles(n) for n in scan.LENGTHS] == [1, 1, 1, 2, 256, 257]


# ------------------------------------------------------------------ the argument check
BASE, STEP = 1 << 28, 1 << 24          # made-up addresses, far enough apart for every array
N, NC, E, D, K, H, S = 100, 120, 1000, 16, 4, 2, 50


def at(slot, offset=0):
    return P(BASE + slot * STEP + offset)


def slots(*names):
    return {name: at(i) for i, name in enumerate(names)}


def max_forward(a):
    return lib.maxk_max_aggregate_forward(a["ptr"], a["idx"], a["sp_data"], 0, a["sp_index"], 0,
                                          a["out"], a["arg_edge"], a["arg_slot"], N, NC, E, D, K,
                                          None)


def heads_forward(a):
    return lib.maxk_heads_aggregate_forward(a["ptr"], a["idx"], a["alpha"], a["sp_data"], 0,
                                            a["sp_index"], 0, a["out"], H, N, NC, E, D, K, None)


def heads_backward(a):
    return lib.maxk_heads_aggregate_backward(a["ptr_t"], a["idx_t"], a["order"], a["alpha"],
                                             a["grad_out"], 0, a["sp_data"], 0, a["sp_index"], 0,
                                             a["grad_sp"], a["grad_alpha"], H, N, NC, E, D, K,
                                             None)


def gat_backward(a):
    return lib.maxk_gat_attention_backward(a["ptr"], a["idx"], a["el"], a["er"], 0.2, a["alpha"],
                                           a["grad_alpha"], a["grad_edge"], a["grad_er"], N, NC,
                                           E, None)


def sample(a):
    return lib.maxk_sample_neighbors(a["ptr"], a["idx"], a["seeds"], a["out_ptr"], a["out_col"],
                                     a["out_eid"], 500, a["scratch"], sp.sample_scratch_bytes(S),
                                     N, E, S, 10, 1, None)


def subgraph_count(a):
    return lib.maxk_induced_subgraph_count(a["ptr"], a["idx"], a["nodes"], a["out_ptr"],
                                           a["counts"], a["scratch"], sg.scratch_bytes(N, S), N,
                                           E, S, None)


def transpose(a):
    return lib.maxk_csr_transpose(a["ptr"], a["idx"], a["val"], a["out_ptr"], a["out_row"],
                                  a["out_order"], a["out_val"], a["scratch"],
                                  tr.scratch_bytes(N, NC, E), N, NC, E, None)


# name -> (call, arrays, an input, an output that must not be NULL (None: every output is
# optional, NULL asks for none), an output, another output of the same call (None: it has one))
ENTRY_POINTS = {
    "maxk_max_aggregate_forward": (
        max_forward, slots("ptr", "idx", "sp_data", "sp_index", "out", "arg_edge", "arg_slot"),
        "sp_data", "out", "out", "arg_edge"),
    "maxk_heads_aggregate_forward": (
        heads_forward, slots("ptr", "idx", "alpha", "sp_data", "sp_index", "out"),
        "alpha", "out", "out", None),
    "maxk_heads_aggregate_backward": (
        heads_backward, slots("ptr_t", "idx_t", "order", "alpha", "grad_out", "sp_data",
                              "sp_index", "grad_sp", "grad_alpha"),
        "order", None, "grad_sp", "grad_alpha"),
    "maxk_gat_attention_backward": (
        gat_backward, slots("ptr", "idx", "el", "er", "alpha", "grad_alpha", "grad_edge",
                            "grad_er"),
        "el", "grad_edge", "grad_edge", "grad_er"),
    "maxk_sample_neighbors": (
        sample, slots("ptr", "idx", "seeds", "out_ptr", "out_col", "out_eid", "scratch"),
        "seeds", "out_col", "out_col", "out_eid"),
    "maxk_induced_subgraph_count": (
        subgraph_count, slots("ptr", "idx", "nodes", "out_ptr", "counts", "scratch"),
        "nodes", "out_ptr", "out_ptr", "counts"),
    "maxk_csr_transpose": (
        transpose, slots("ptr", "idx", "val", "out_ptr", "out_row", "out_order", "out_val",
                         "scratch"),
        "idx", "out_row", "out_row", "out_order"),
}
NULL_TEXT = "null pointer"
OVERLAP_TEXT = "an output overlaps an input or another output"


def refused(name, call, arrays, text):
    got = call(arrays)
    message = lib.maxk_last_error().decode()
    assert got == INVALID and message == f"{name}: {text}", (name, got, message)


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_one_argument_check_behind_every_file(name):
    call, arrays, an_input, needed_output, output, other_output = ENTRY_POINTS[name]
    refused(name, call, dict(arrays, **{an_input: None}), NULL_TEXT)
    if needed_output:
        refused(name, call, dict(arrays, **{needed_output: None}), NULL_TEXT)
    # an output that starts inside an input, and one that starts inside another output
    refused(name, call, dict(arrays, **{output: P(arrays[an_input].value + 4)}), OVERLAP_TEXT)
    if other_output:
        refused(name, call, dict(arrays, **{other_output: P(arrays[output].value + 4)}),
                OVERLAP_TEXT)
