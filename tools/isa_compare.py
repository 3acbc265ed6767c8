#!/usr/bin/env python3
"""Compares the gfx950 kernels of two assembly directories, kernel by kernel.

    tools/isa_compare.py OLD_DIR NEW_DIR [--names TABLE]

Each directory holds the `hipcc <build.FLAGS without -fPIC -shared> --cuda-device-only -S` output (*.s) of the lighting translation
units of one revision.  For every kernel one line: name, instruction count, `equal` or `differs`.  Equal means the same kernel
descriptor (every .amdhsa_* line: registers, LDS, scratch, kernarg size) and the same instruction stream after three
normalisations: comments stripped, mangled symbols replaced by one token, .LBB<n>_ renumbered.  TABLE renames kernels between the
revisions: lines `old -> new`, names as c++filt prints them without the return type, `cry::` and the argument list.
Exit status 1 if any kernel differs or has no partner.
"""
import glob
import os
import re
import subprocess
import sys


def short_names(mangled):
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    names = {}
    for m, d in zip(mangled, out):
        d = d[:d.rindex(">(") + 1] if ">(" in d else d[:d.index("(")]       # kernels return void: no function type in the arguments
        names[m] = re.sub(r"^void ", "", d).replace("cry::", "")
    return names


def kernels(directory):
    """{short name: (instruction stream, descriptor)} of every kernel of the directory's *.s files."""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        starts = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m}
        for i, l in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
            if not m:
                continue
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            desc = [x.strip() for x in lines[i + 1:end]]
            stream = []
            for x in lines[starts[m.group(1)] + 1:i]:
                x = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", x.split(";")[0])).strip()
                if x.startswith(".section"):
                    break
                if x:
                    stream.append(x)
            found[m.group(1)] = (stream, desc)
    names = short_names(list(found))
    return {names[m]: v for m, v in found.items()}


def main(argv):
    if len(argv) not in (3, 5) or (len(argv) == 5 and argv[3] != "--names"):
        sys.exit(__doc__)
    old, new = kernels(argv[1]), kernels(argv[2])
    renamed = {}
    if len(argv) == 5:
        for l in open(argv[4]):
            if "->" in l and not l.startswith("#"):
                a, b = l.split("->")
                renamed[a.strip()] = b.strip()
    bad = 0
    for name in sorted(old):
        target = renamed.get(name, name)
        if target not in new:
            print("%-110s %6s  no partner" % (name, "-"))
            bad += 1
            continue
        (s0, d0), (s1, d1) = old[name], new.pop(target)
        count = sum(1 for x in s1 if not x.endswith(":") and not x.startswith("."))
        verdict = "equal" if (s0, d0) == (s1, d1) else "differs (%s)" % ", ".join(
            w for w, same in (("instructions", s0 == s1), ("descriptor", d0 == d1)) if not same)
        bad += verdict != "equal"
        print("%-110s %6d  %s" % (target if target == name else "%s  [was %s]" % (target, name), count, verdict))
    for name in sorted(new):
        print("%-110s %6s  no partner (new)" % (name, "-"))
        bad += 1
    print("%d kernels compared, %d differ or lack a partner" % (len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
