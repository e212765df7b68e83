#!/usr/bin/env python3
"""Per-kernel A/B of two device assembly files of the same source (tools/asmstat.sh's approach, for every kernel and both sides):
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -S --cuda-device-only FILE.hip -o FILE.s      (parent and new)
    tools/asm_ab.py parent.s new.s [--gone REGEX]
Prints, per kernel, the resources of the code object's metadata, the counts of six instruction classes and the instruction total of
both sides, the opcodes whose counts moved, and which kernels exist on one side only.  Exit status 1 if a kernel of both sides
differs in a resource or a class count, or if the kernels that left are not exactly those --gone matches."""
import collections
import re
import sys

RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")
CLASSES = (("mfma", r"v_mfma_"), ("ds_read", r"ds_read"), ("ds_write", r"ds_write"), ("vmem_load", r"(global|buffer)_load"),
           ("vmem_store", r"(global|buffer)_store"), ("f64_fma_mul_add", r"v_(fma|mul|add)_f64"))


def kernels(path):
    """{mangled name: (resources, Counter of opcodes)}"""
    text = open(path).read()
    meta = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = tuple(int(re.search(rf"\.{r}:\s+(\d+)", block).group(1)) for r in RESOURCES)
    out = {}
    for name in meta:
        body = text[text.index(f"\n{name}:") : text.index(f".Lfunc_end", text.index(f"\n{name}:"))]
        ops = collections.Counter()
        for line in body.splitlines():
            m = re.match(r"\t([a-z][a-z0-9_]+)(\s|$)", line)
            if m:
                ops[m.group(1)] += 1
        out[name] = (meta[name], ops)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    gone_re = sys.argv[sys.argv.index("--gone") + 1] if "--gone" in sys.argv else None
    bad = 0
    print(f"parent: {len(a)} kernels   new: {len(b)} kernels")
    print("columns: " + " ".join(RESOURCES) + " | " + " ".join(c for c, _ in CLASSES) + " | instructions")
    for name in sorted(a):
        ra, oa = a[name]
        ca = tuple(sum(n for op, n in oa.items() if re.match(p, op)) for _, p in CLASSES)
        line = f"{name}\n    parent {' '.join(map(str, ra))} | {' '.join(map(str, ca))} | {sum(oa.values())}"
        if name not in b:
            ok = gone_re is not None and re.search(gone_re, name)
            bad += not ok
            print(line + ("\n    new    (not built any more)" if ok else "\n    new    MISSING"))
            continue
        rb, ob = b[name]
        cb = tuple(sum(n for op, n in ob.items() if re.match(p, op)) for _, p in CLASSES)
        same = ra == rb and ca == cb
        bad += not same
        print(line + f"\n    new    {' '.join(map(str, rb))} | {' '.join(map(str, cb))} | {sum(ob.values())}   "
              + ("equal" if same and oa == ob else "resources and classes equal" if same else "DIFFERENT"))
        moved = {op: (oa[op], ob[op]) for op in sorted(set(oa) | set(ob)) if oa[op] != ob[op]}
        if moved:
            print("    moved: " + ", ".join(f"{op} {x}->{y}" for op, (x, y) in moved.items()))
    for name in sorted(set(b) - set(a)):
        bad += 1
        print(f"{name}\n    parent (none)   NEW KERNEL")
    if gone_re is not None:
        for name in sorted(b):
            if re.search(gone_re, name):
                bad += 1
                print(f"{name}\n    still built, expected gone")
    print(f"verdict: {'every kernel of both sides equal in resources and instruction classes' if not bad else f'{bad} findings'}; "
          f"{len(set(a) - set(b))} kernels left, {len(set(b) - set(a))} came")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
