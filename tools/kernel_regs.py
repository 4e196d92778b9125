#!/usr/bin/env python3
"""Registers and scratch of every kernel, one tree against another (diagnostic;
profiles/*/registers.txt).

Reads the code-object metadata (amdhsa.kernels: .vgpr_count, .agpr_count,
.sgpr_count, .private_segment_fixed_size) out of the ISA listings that
`make isa` leaves under build/isa of each tree and prints every kernel whose
figures differ, the kernels only one tree has, and those that gained scratch.

  python tools/kernel_regs.py PARENT_TREE/build/isa build/isa
"""
import glob
import os
import re
import sys

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size")


def kernels(isa_dir):
    out = {}
    for path in sorted(glob.glob(os.path.join(isa_dir, "*.s"))):
        text = open(path).read()
        meta = text[text.rindex("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
        for entry in re.split(r"\n  - ", meta)[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry)
            vals = [re.search(rf"{re.escape(k)}:\s+(\d+)", entry) for k in KEYS]
            if name and all(vals):
                out[name.group(1)] = tuple(int(v.group(1)) for v in vals)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    both = sorted(set(a) & set(b))
    changed = [k for k in both if a[k] != b[k]]
    gained = [k for k in both if a[k][3] == 0 and b[k][3] > 0]
    print(f"# .vgpr_count / .agpr_count / .sgpr_count / .private_segment_fixed_size of every kernel, parent -> branch "
          f"(code-object metadata, gfx950); kernels not listed are unchanged")
    print(f"# {len(a)} -> {len(b)} kernels; only in the branch: {sorted(set(b) - set(a))}; only in the parent: "
          f"{sorted(set(a) - set(b))}; changed: {len(changed)}")
    print(f"# kernels with zero scratch in the parent and scratch in the branch: {gained}")
    print(f"# kernels with scratch: parent {sum(1 for k in a if a[k][3])}, branch {sum(1 for k in b if b[k][3])}; "
          f"whose scratch changed: {[k for k in both if a[k][3] != b[k][3]]}")
    for k in changed:
        x, y = a[k], b[k]
        print(f"VGPR {x[0]} -> {y[0]} agpr {x[1]} -> {y[1]} sgpr {x[2]} -> {y[2]} scratch {x[3]} -> {y[3]} {k}")
    return 1 if gained else 0


if __name__ == "__main__":
    sys.exit(main())
