"""CPU: the variant tables of csrc/variants.h are the fixture's instantiations of their kernel
families, and the selectors stay inside them. build/variant_check (tools/variant_check.cpp, built
by `make` with the host compiler) walks every selector's input domain: each selected variant is in
its family's table, each table entry is selected by some input; it prints the tables' kernel
names as tests/golden/kernel_instantiations.txt lists them. The launchers instantiate kernels
from those tables alone, so with tests/test_kernel_list.py (fixture == library) the source and
the library state the same set."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations.txt")
CHECK = os.path.join(os.path.dirname(HERE), "spgemm-gnn_amd", "build", "variant_check")
FAMILIES = ("spgemm_fwd_kernel", "cbsr_stats4_kernel", "pack_cbsr3_kernel", "sspmm_bwd4_kernel",
            "sspmm_bwd_rows_kernel", "topk_exact_kernel", "topk_ref_compat_kernel",
            "maxk_scatter_backward_kernel", "sddmm_edge_grad_kernel", "dense_spmm_kernel")


def test_selectors_stay_in_the_tables_and_the_tables_are_the_fixture():
    if not os.path.exists(CHECK):
        pytest.skip("spgemm-gnn_amd/build/variant_check is not built (make -C spgemm-gnn_amd)")
    run = subprocess.run([CHECK], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr
    with open(FIXTURE) as f:
        want = [ln.strip() for ln in f
                if ln.strip().startswith(tuple("maxk::" + k + "<" for k in FAMILIES))]
    assert run.stdout.splitlines() == want
