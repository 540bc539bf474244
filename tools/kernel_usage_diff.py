#!/usr/bin/env python3
"""Per translation unit: register, scratch and LDS usage of every kernel in two builds of csrc/, from the code objects' metadata.

    python tools/kernel_usage_diff.py <csrc of build A> <csrc of build B> [allowed-removal regex]

Both directories hold the objects the project Makefile leaves behind (bluestein.o, pfa.o, ...).  The gfx950 code object of each
is taken out of its .hip_fatbin section and the amdhsa.kernels notes are compared kernel by kernel (mangled name).  No GPU needed.
Kernels only in A are listed; they must match the regex (on the demangled name) when one is given.  Exit status 1 on a difference.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
UNITS = ["bluestein", "pfa", "peaks", "sim", "bootstrap", "solve", "resample", "pal_api"]
FIELDS = [".sgpr_count", ".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
          ".sgpr_spill_count", ".vgpr_spill_count"]


def kernels(obj, tmp):
    fatbin, code = os.path.join(tmp, "unit.hipfb"), os.path.join(tmp, "unit.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, obj], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fatbin,
                    "--output=" + code, "--unbundle"], check=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", code], check=True, capture_output=True, text=True).stdout
    found, cur, inside = [], None, False
    for line in notes.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif re.match(r"^amdhsa\.\w+:", line):
            inside = False
        elif inside:
            if line.startswith("  - "):                              # first key of the next kernel
                cur = {}
                found.append(cur)
            m = re.match(r"^  (?:- |  )(\.\w+):\s*(.*)$", line)      # (the keys of .args entries are indented further)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2)
    return {k[".name"]: tuple(k.get(f, "?") for f in FIELDS) for k in found}


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    allowed = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    ok = True
    print("per kernel:", " ".join(FIELDS))
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:
            a, b = kernels(os.path.join(a_dir, unit + ".o"), tmp), kernels(os.path.join(b_dir, unit + ".o"), tmp)
            both = sorted(set(a) & set(b))
            differ = [k for k in both if a[k] != b[k]]
            gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            print(f"== {unit}: A {len(a)} kernels, B {len(b)}, in both {len(both)}, differing {len(differ)}, only in A {len(gone)}, only in B {len(new)}")
            for k in differ:
                ok = False
                print("  DIFFERS", demangle(k), " ".join(a[k]), "|", " ".join(b[k]))
            for k in new:
                ok = False
                print("  ONLY IN B", demangle(k), " ".join(b[k]))
            for k in gone:
                name = demangle(k)
                fine = allowed is None or allowed.search(name) is not None
                ok = ok and fine
                print("  only in A" if fine else "  UNEXPECTEDLY ONLY IN A", name, " ".join(a[k]))
    print("VERDICT:", "every kernel present in both builds has identical usage; nothing new, nothing unexpected gone" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
