#!/usr/bin/env python3
"""Kernel by kernel, the gfx950 assembly of every HIP source of the default build in this tree against another tree (a checkout of the
parent commit, say): which kernels are instruction for instruction the same, and for every kernel its instruction count, registers,
LDS, scratch, spills and place in the file.  Cross-compiles only; no GPU.

    python scripts/isa_compare.py OTHER_TREE

Both trees' sources (build.py's SOURCES that end in .hip; one the other tree lacks is listed with its figures) are compiled with
build.py's FLAGS plus -S --cuda-device-only.  Comments and
the .file / .ident / .loc lines are dropped and local labels lose the ordinal of their function; what is left of a kernel's body (instructions, labels, directives) is compared as text.
The figures come from the kernels' metadata records at the end of the assembly."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from divans_amd import build as dbuild  # noqa: E402

SOURCES = tuple(s for s in dbuild.SOURCES if s.endswith(".hip"))
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def assembly(tree, src, tmp, tag):
    out = os.path.join(tmp, f"{tag}_{src}.s")
    subprocess.run([dbuild.hipcc()] + dbuild.FLAGS + ["-S", "--cuda-device-only", "-x", "hip", os.path.join(tree, "divans_amd", "csrc", src), "-o", out],
                   check=True, capture_output=True, text=True)
    lines = []
    for l in open(out):
        l = re.split(r";|//", l, 1)[0].rstrip()
        if l.strip() and not re.match(r"\s*\.(file|ident|loc)\b", l):
            # local labels carry the ordinal of their function in the file (.LBB12_3): a kernel added in front renumbers the ones behind it
            lines.append(re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", l))
    return lines


def kernels(lines):
    """[(name, body lines, metadata)] in file order."""
    meta, rec = {}, {}
    for l in lines[lines.index("amdhsa.kernels:") + 1:]:       # one record per kernel, its keys four columns in
        m = re.match(r"  [- ] \.(\w+):\s*(\S+)$", l)
        if l.startswith("  - ") or not l.startswith("  "):
            rec = {}
        if m and m.group(1) == "name":
            meta[m.group(2)] = rec
        elif m and m.group(1) in FIELDS:
            rec[m.group(1)] = int(m.group(2))
    found = []
    for i, l in enumerate(lines):
        if l.endswith(":") and l[:-1] in meta:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            found.append((l[:-1], lines[i + 1:end], meta[l[:-1]]))
    return found


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"^void |divans_hip::|\(.*$", "", d) for n, d in zip(names, res)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def n_instructions(body):
    return sum(1 for l in body if not l.endswith(":") and not l.lstrip().startswith("."))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    other = os.path.abspath(sys.argv[1])
    out = ["kernel: identical to OTHER_TREE or not | instructions | vgpr | sgpr | LDS bytes (static) | scratch bytes | sgpr spills | vgpr spills | place in file",
           "(a figure that differs from the other tree's is followed by the other tree's in brackets)", ""]
    with tempfile.TemporaryDirectory() as tmp:
        for src in SOURCES:
            have = os.path.exists(os.path.join(other, "divans_amd", "csrc", src))
            mine, theirs = kernels(assembly(ROOT, src, tmp, "this")), (kernels(assembly(other, src, tmp, "other")) if have else [])
            nice = demangle([k[0] for k in mine])
            their_place = {k[0]: i for i, k in enumerate(theirs)}
            common = [k[0] for k in mine if k[0] in their_place]
            out.append(f"{src}: {len(mine)} kernels, {len(theirs)} in the other tree; order of the ones both hold " +
                       ("unchanged" if common == [k[0] for k in theirs] else "CHANGED") +
                       f"; identical: {sum(1 for n, b, _ in mine if n in their_place and b == theirs[their_place[n]][1])}")
            for i, (name, body, meta) in enumerate(mine):
                if name not in their_place:
                    out.append(f"  {nice[name]:44s} {'new':9s} | " + " | ".join([str(n_instructions(body))] + [str(meta.get(f)) for f in FIELDS] + [str(i + 1)]))
                    continue
                j = their_place[name]
                _, obody, ometa = theirs[j]
                both = lambda a, b: f"{a}" if a == b else f"{a} [{b}]"
                cols = [both(n_instructions(body), n_instructions(obody))] + [both(meta.get(f), ometa.get(f)) for f in FIELDS] + [both(i + 1, j + 1)]
                out.append(f"  {nice[name]:44s} {'identical' if body == obody else 'DIFFERENT':9s} | " + " | ".join(cols))
            out.append("")
    print("\n".join(out))


if __name__ == "__main__":
    main()
