"""CPU: tests/golden/kernel_instantiations.txt is the list of kernel instantiations compiled into
the built libmaxk_hip.so (tools/kernel_list.py). A change that adds, removes or re-parameterises an
instantiation has to touch the fixture, and tests/test_gpu_kernel_variants.py then demands a case
that launches it."""
import importlib.util
import os

import pytest

import maxk_kernels as mk

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations.txt")


def _tool():
    path = os.path.join(os.path.dirname(HERE), "tools", "kernel_list.py")
    spec = importlib.util.spec_from_file_location("kernel_list", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


kernel_list = _tool()


def test_fixture_is_sorted_unique_and_ours():
    names = kernel_list.read_list(FIXTURE)
    assert names == sorted(set(names))
    assert all(n.startswith("maxk::") and "(" not in n for n in names)


def test_fixture_equals_the_built_library():
    if kernel_list.find_readelf() is None:
        pytest.skip("no llvm-readelf to list the library's symbols with")
    built = kernel_list.compiled(mk.LIB_PATH)
    want = kernel_list.read_list(FIXTURE)
    added, gone = sorted(set(built) - set(want)), sorted(set(want) - set(built))
    assert not added and not gone, (
        f"the library holds {len(built)} instantiations, the fixture {len(want)}.\n"
        f"compiled but not in the fixture ({len(added)}):\n  " + "\n  ".join(added) +
        f"\nin the fixture but not compiled ({len(gone)}):\n  " + "\n  ".join(gone) +
        "\nregenerate with: python tools/kernel_list.py > tests/golden/kernel_instantiations.txt")


def test_strip_params_on_demangled_forms():
    strip = kernel_list.strip_params
    assert strip("void maxk::sspmm_bwd4_kernel<8, 512, 4, true, true>(maxk::BwdTask const*, "
                 "float*)") == "maxk::sspmm_bwd4_kernel<8, 512, 4, true, true>"
    assert strip("maxk::iota_kernel(int, int*)") == "maxk::iota_kernel"
    assert strip('"void maxk::f<(int)3>(int) [clone .kd]"') == "maxk::f<(int)3>"
    assert strip("maxk::iota_kernel(int, int*) (.kd)") == "maxk::iota_kernel"


def test_launched_reads_a_stats_csv(tmp_path):
    csv = tmp_path / "stats.csv"
    csv.write_text('"Name","Calls","TotalDurationNs"\n'
                   '"void maxk::iota_kernel(int, int*)",3,100\n'
                   '"maxk::dense_spmm_kernel<4, 4>(int const*, float*)",1,50\n'
                   '"void rocprim::detail::trampoline_kernel<int>(int)",9,10\n'
                   '"__amd_rocclr_fillBufferAligned.kd",2,5\n')
    assert kernel_list.launched(str(csv)) == ["maxk::dense_spmm_kernel<4, 4>",
                                              "maxk::iota_kernel"]
