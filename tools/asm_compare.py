#!/usr/bin/env python3
"""Compare the kernels of two sets of device assembly files, text against text.

A refactor that only moves device code between files must leave every
kernel's machine code as it was.  Compile the .hip files of both trees
device-only to assembly with the Makefile's flags,

    hipcc $(HIPFLAGS) --cuda-device-only -S -o old/prk_spans.s csrc/prk_spans.hip
    (prk_kernels.hip with $(KERNEL_SCHED) as well)

and run

    tools/asm_compare.py --old old/*.s --new new/*.s

A kernel is what has an .amdhsa_kernel descriptor.  Its text is everything
from its label to the end of its "Kernel info" comments: the instruction
stream, the descriptor block, the .set lines with its register, LDS and
scratch numbers, and the compiler's summary of them.  Kernels are matched by
name across all files of a set, whichever file they are in.  Only what
depends on a kernel's position in its file is normalised: the function
number in local labels (.LBB12_3, .Lfunc_end12, .LJTI12_0, .Ltmp12) and the
__hip_cuid_* symbol.

Prints the kernels that differ, are missing or are new, with the first
differing line of each, and exits 1 if there are any (2 for a file without
kernels); else prints the count and exits 0.
"""
import argparse
import re
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end|tmp)(\d+)")
BLOCK = re.compile(r"\bBB\d+_(\d+)")  # the compiler's comments name blocks without the .L
CUID = re.compile(r"__hip_cuid_\w+")
PAD = re.compile(r"[ \t]+;")  # (a comment's column moves with the width of the label before it)


def normalise(line):
    line = LOCAL.sub(lambda m: ".L%s#" % m.group(1), line)
    line = BLOCK.sub(lambda m: "BB#_%s" % m.group(1), line)
    return PAD.sub(" ;", CUID.sub("__hip_cuid_#", line)).rstrip()


def kernels_of(path):
    """{kernel name: its normalised lines} of one assembly file."""
    lines = open(path, errors="replace").read().split("\n")
    out = {}
    i, n = 0, len(lines)
    while i < n:
        m = LABEL.match(lines[i])
        if not m or m.group(1).startswith(".L"):
            i += 1
            continue
        name, j, is_kernel, in_info = m.group(1), i + 1, False, False
        while j < n:
            s = lines[j]
            if s.startswith("\t.amdhsa_kernel " + name):
                is_kernel = True
            if ".AMDGPU.csdata" in s:
                in_info = True
            elif in_info and not s.startswith(";"):
                break
            elif LABEL.match(s) and not s.startswith(".L"):
                break  # (a symbol that is no function: the next label ends it)
            j += 1
        if is_kernel:
            if name in out:
                sys.exit("%s: kernel %s defined twice" % (path, name))
            out[name] = [normalise(s) for s in lines[i:j]]
        i = j
    return out


def collect(paths):
    allk = {}
    for p in paths:
        ks = kernels_of(p)
        if not ks:
            print("%s: no kernels found" % p)
            sys.exit(2)
        for k, v in ks.items():
            if k in allk:
                sys.exit("kernel %s is in %s and in %s" % (k, allk[k][0], p))
            allk[k] = (p, v)
    return allk


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True, help="assembly files of the parent")
    ap.add_argument("--new", nargs="+", required=True, help="assembly files of the change")
    a = ap.parse_args()
    old, new = collect(a.old), collect(a.new)
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in new:
            print("MISSING  %s (was in %s)" % (k, old[k][0]))
        elif k not in old:
            print("NEW      %s (in %s)" % (k, new[k][0]))
        elif old[k][1] != new[k][1]:
            o, w = old[k][1], new[k][1]
            at = next((q for q in range(min(len(o), len(w))) if o[q] != w[q]), min(len(o), len(w)))
            print("DIFFERS  %s (%s -> %s), %d -> %d lines, first at line %d of the kernel:" %
                  (k, old[k][0], new[k][0], len(o), len(w), at + 1))
            print("    old: %s" % (o[at] if at < len(o) else "<end>"))
            print("    new: %s" % (w[at] if at < len(w) else "<end>"))
        else:
            continue
        bad += 1
    print("%d kernels compared, %d differing" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
