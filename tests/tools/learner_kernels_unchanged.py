#!/usr/bin/env python3
"""Are the single-learner kernels of armenv::learner:: the same machine code in two builds of libarmenv.so?  (No GPU needed.)

  python tests/tools/learner_kernels_unchanged.py <libarmenv.so of the parent commit> [<libarmenv.so of this tree>]

Compares, kernel by kernel, the llvm-objdump disassembly (mnemonic and operands of every instruction, in order; branch operands are
PC-relative, so code that moved compares equal) and the resource metadata (registers, scratch, LDS) of every learner kernel that
both libraries hold, and lists the kernels that only one of them holds.  Prints a report; exit status 1 if a shared kernel differs."""
import sys

import isa


def _text(ins):
    """instruction texts up to the kernel's last s_endpgm: what follows is the padding between kernels and after the last one"""
    text = [i.text for i in ins]
    ends = [k for k, i in enumerate(ins) if i.mnem == "s_endpgm"]
    return text[:ends[-1] + 1] if ends else text


def learner_kernels(lib):
    return {dm.split("armenv::learner::")[1].split("(")[0]: (md, _text(ins))
            for _, dm, md, ins in isa.all_kernels(lib) if "armenv::learner::" in dm}


def main(argv):
    old, new = learner_kernels(argv[0]), learner_kernels(argv[1] if len(argv) > 1 else isa.LIB)
    changed = 0
    for name in sorted(old):
        if name not in new:
            print("%-28s MISSING from the new build" % name)
            changed += 1
            continue
        (md0, t0), (md1, t1) = old[name], new[name]
        same = t0 == t1 and md0 == md1
        changed += not same
        print("%-28s %s  %5d instructions, vgpr %d agpr %d sgpr %d lds %d scratch %d" % (
            name, "identical" if same else "DIFFERENT", len(t1), md1["vgpr"], md1["agpr"], md1["sgpr"], md1["lds"], md1["scratch"]))
        if not same:
            first = next((k for k, (x, y) in enumerate(zip(t0, t1)) if x != y), min(len(t0), len(t1)))
            print("    %d -> %d instructions; first difference at instruction %d; metadata %s -> %s" % (len(t0), len(t1), first, md0, md1))
    for name in sorted(set(new) - set(old)):
        md, t = new[name]
        print("%-28s new        %5d instructions, vgpr %d agpr %d sgpr %d lds %d scratch %d" % (
            name, len(t), md["vgpr"], md["agpr"], md["sgpr"], md["lds"], md["scratch"]))
    print("%d of %d kernels of the old build differ" % (changed, len(old)))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
