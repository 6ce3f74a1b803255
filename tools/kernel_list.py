#!/usr/bin/env python3
"""The kernel instantiations compiled into libmaxk_hip.so, and the ones a profiled run launched.

  tools/kernel_list.py [LIB]             demangled names of the library's maxk:: kernels, sorted,
                                         one per line, without parameter lists (the fixture
                                         tests/golden/kernel_instantiations.txt is this output)
  tools/kernel_list.py --launched CSV..  the maxk:: kernel names of kernel-stats CSVs
                                         (rocprofv3 --kernel-trace --stats), in the same form
  tools/kernel_list.py --launched CSV.. --diff FIXTURE
                                         both differences against a list; exit 1 unless equal
  --namespace PREFIX                     keep the names that start with PREFIX instead of maxk::
                                         (maxk_mh:: -> tests/golden/kernel_instantiations_heads.txt)

The compiled set comes from the host stub symbols (`__device_stub__`) in the library's symbol
table, read with llvm-readelf and demangled with c++filt; kernels outside namespace maxk
(rocprim's trampolines) are dropped.
"""
import argparse
import csv
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "spgemm-gnn_amd", "maxk_kernels", "libmaxk_hip.so")
STUB = "__device_stub__"


def find_readelf():
    """llvm-readelf of the ROCm toolchain or of PATH; None when there is none."""
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin",
                              "llvm-readelf"),
                 shutil.which("llvm-readelf")):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def strip_params(name):
    """`void maxk::f<8, true>(int, float*) [clone .kd]` -> `maxk::f<8, true>`: the name up to
    the parameter list, i.e. the first '(' outside template angle brackets."""
    name = name.strip().strip('"')
    name = re.sub(r"\s*\[clone [^\]]*\]$", "", name)
    if name.endswith(".kd"):
        name = name[:-3]
    depth, out = 0, []
    for ch in name:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        out.append(ch)
    name = "".join(out).strip()
    if name.startswith("void "):
        name = name[5:]
    return name


DEFAULT_PREFIX = "maxk::"


def ours(names, prefix=DEFAULT_PREFIX):
    return sorted({n for n in map(strip_params, names) if n.startswith(prefix)})


def compiled(lib=DEFAULT_LIB, readelf=None, prefix=DEFAULT_PREFIX):
    """Sorted names of the kernel instantiations of namespace `prefix` (maxk::) in `lib`."""
    readelf = readelf or find_readelf()
    if readelf is None:
        raise FileNotFoundError("llvm-readelf not found")
    sym = subprocess.run([readelf, "--symbols", "--wide", lib], check=True, capture_output=True,
                         text=True).stdout
    mangled = sorted({w for line in sym.splitlines() for w in line.split()[-1:]
                      if STUB in w})
    dem = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", check=True,
                         capture_output=True, text=True).stdout
    return ours((n.replace(STUB, "") for n in dem.splitlines() if n.strip()), prefix)


def launched(csv_path, prefix=DEFAULT_PREFIX):
    """Sorted maxk:: kernel names of a kernel-stats CSV (column "Name", else the first)."""
    with open(csv_path, newline="") as f:
        rows = list(csv.reader(f))
    if not rows:
        return []
    head = [h.strip().strip('"') for h in rows[0]]
    col = head.index("Name") if "Name" in head else head.index("KernelName") \
        if "KernelName" in head else 0
    return ours((r[col] for r in rows[1:] if len(r) > col), prefix)


def read_list(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("lib", nargs="?", default=DEFAULT_LIB)
    ap.add_argument("--launched", metavar="CSV", nargs="+",
                    help="kernel-stats CSVs of traced runs (several: the union)")
    ap.add_argument("--diff", metavar="LIST", help="compare with a list of names")
    ap.add_argument("--namespace", metavar="PREFIX", default=DEFAULT_PREFIX,
                    help="keep the names that start with PREFIX (default maxk::)")
    a = ap.parse_args(argv)
    if a.launched:
        names = sorted({n for path in a.launched for n in launched(path, a.namespace)})
    else:
        names = compiled(a.lib, prefix=a.namespace)
    if not a.diff:
        print("\n".join(names))
        return 0
    want = set(read_list(a.diff))
    got = set(names)
    for n in sorted(got - want):
        print("+ " + n)
    for n in sorted(want - got):
        print("- " + n)
    print(f"{len(got)} names, {len(want)} in {a.diff}: " +
          ("equal" if got == want else f"{len(got - want)} extra, {len(want - got)} missing"))
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
