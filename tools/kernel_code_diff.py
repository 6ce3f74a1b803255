#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, function by function.

    tools/kernel_code_diff.py A B          A, B: repository roots (for example two checkouts)

Every spgemm-gnn_amd/csrc/*.hip of each tree is compiled with the Makefile's FLAGS plus
--offload-device-only -c, the hipv4-amdgcn-amd-amdhsa--gfx950 object is unbundled and
disassembled (llvm-objdump -d --no-show-raw-insn; addresses, trailing // comments and the s_nop
padding behind a function dropped, which is longest behind whichever function comes last) and
keyed by function name; llvm-readelf --notes gives each kernel's register counts, LDS, scratch and
kernarg sizes. Prints the names whose instruction lists or resources differ, or that only one
tree has, and exits non-zero if there are any. The order of emission in the object is not
compared: it follows the order of instantiation in the source.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
LLVM = os.path.join(ROCM, "llvm", "bin")
ARCH = "gfx950"
TARGET = "hipv4-amdgcn-amd-amdhsa--" + ARCH
META = (".sgpr_count", ".vgpr_count", ".agpr_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size",
        ".sgpr_spill_count", ".vgpr_spill_count", ".wavefront_size")


def make_flags(root):
    """FLAGS of the tree's Makefile, make variables expanded."""
    text = open(os.path.join(root, "spgemm-gnn_amd", "Makefile")).read().replace("\\\n", " ")
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", ARCH).split()


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, text=True).stdout


def functions(obj):
    """{function: [instruction lines]} of a code object."""
    out, cur = {}, None
    for ln in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip() not in ("", "..."):  # "...": padding between functions
            cur.append(re.sub(r"\s*//.*$", "", ln).strip())
    for body in out.values():  # alignment padding behind a function: longest behind the last one
        while body and body[-1] == "s_nop 0":
            body.pop()
    return out


def resources(obj):
    """{kernel: {field: value}} from the amdhsa.kernels list of the code object's metadata note:
    a kernel starts at "  - .field:", its own fields sit at that depth (4 columns)."""
    out, cur = {}, None
    for ln in run(os.path.join(LLVM, "llvm-readelf"), "--notes", obj).splitlines():
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3)
            if m.group(2) == ".name":
                out[m.group(3)] = cur
    return {name: {k: f.get(k) for k in META} for name, f in out.items()}


def tree(root, work):
    funcs, res = {}, {}
    csrc = os.path.join(root, "spgemm-gnn_amd", "csrc")
    for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        base = os.path.join(work, os.path.basename(src)[:-4])
        run(HIPCC, *make_flags(root), "--offload-device-only", "-c", src, "-o", base + ".bundle",
            cwd=os.path.join(root, "spgemm-gnn_amd"))
        run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
            "--targets=" + TARGET, "--input=" + base + ".bundle", "--output=" + base + ".co")
        for name, body in functions(base + ".co").items():
            funcs[os.path.basename(src) + ": " + name] = body
        for name, r in resources(base + ".co").items():
            res[os.path.basename(src) + ": " + name] = r
    return funcs, res


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
        fa, ra = tree(os.path.abspath(sys.argv[1]), wa)
        fb, rb = tree(os.path.abspath(sys.argv[2]), wb)
    bad = 0
    for what, a, b in (("code", fa, fb), ("resources", ra, rb)):
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                print(f"{what}: only in {'B' if name not in a else 'A'}: {name}")
                bad += 1
            elif a[name] != b[name]:
                print(f"{what}: differs: {name}")
                bad += 1
    print(f"{len(fa)} / {len(fb)} functions, {len(ra)} / {len(rb)} kernels with metadata, "
          f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
