#!/usr/bin/env python3
"""Are the trajectory store's single kernels (her_sample_kernel<6>, <9>, index_episodes_kernel) the same machine code in two builds
of libarmenv.so, now that they share their bodies with the population kernels?  (No GPU needed.)

  python tests/tools/pop_store_kernels_unchanged.py <libarmenv.so of the parent commit> [<libarmenv.so of this tree>]

The comparison of learner_kernels_unchanged.py -- the instruction texts in order up to the last s_endpgm, and the resource metadata
-- over the kernels of csrc/armenv_replay.h.  Prints a report; exit status 1 if a kernel both builds hold differs."""
import sys

import isa
from learner_kernels_unchanged import _text


def store_kernels(lib):
    return {dm.replace("void ", "").split("(")[0].replace("armenv::", ""): (md, _text(ins))
            for _, dm, md, ins in isa.all_kernels(lib) if "her_sample" in dm or "index_episodes" in dm}


def main(argv):
    old, new = store_kernels(argv[0]), store_kernels(argv[1] if len(argv) > 1 else isa.LIB)
    changed = 0
    for name in sorted(set(old) | set(new)):
        if name not in new:
            print("%-30s MISSING from the new build" % name)
            changed += 1
            continue
        md, t = new[name]
        state = "new" if name not in old else ("identical" if old[name] == new[name] else "DIFFERENT")
        changed += state == "DIFFERENT"
        print("%-30s %-9s %5d instructions, vgpr %d agpr %d sgpr %d lds %d scratch %d spilled vgprs %d" % (
            name, state, len(t), md["vgpr"], md["agpr"], md["sgpr"], md["lds"], md["scratch"], md["spill_vgpr"]))
        if state == "DIFFERENT":
            md0, t0 = old[name]
            first = next((k for k, (x, y) in enumerate(zip(t0, t)) if x != y), min(len(t0), len(t)))
            print("    %d -> %d instructions; first difference at instruction %d; metadata %s -> %s" % (len(t0), len(t), first, md0, md))
    print("%d of %d kernels of the old build differ" % (changed, len(old)))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
