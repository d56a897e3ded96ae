#!/usr/bin/env python3
"""Which kernels are the same machine code in two builds of libarmenv.so, and how do the others differ?  (No GPU needed.)

  python tests/tools/kernels_unchanged.py [--match REGEX] <libarmenv.so of the parent commit> [<libarmenv.so of this tree>]

Compares, kernel by kernel (demangled name; --match keeps the names the regex finds), the llvm-objdump disassembly -- mnemonic and
operands of every instruction up to the last s_endpgm, in order -- and the resource metadata of both builds (vgpr, agpr, sgpr,
scratch, lds, spilled vgprs).  A kernel is

  identical     same instruction texts, same metadata;
  re-allocated  the same mnemonics the same number of times, in other registers or another order;
  DIFFERENT     another instruction multiset: the count delta is printed;

and for the last two every resource that went up is named and the instruction mix (isa.mix) of every innermost loop
(isa.innermost_loops: the IK trip of the env kernels) is compared as well.  Kernels only one build holds are listed; a table per kernel
family closes the report.

Exit status 1 if a kernel differs, or is missing from the new build, that is not built from the lanes of csrc/armenv_env.h (the env
step / rollout / reset / summary families, LANE_KERNELS): a change to the lanes has no business in the others.  The checks earlier
changes ran with scripts of their own:
  --match 'armenv::learner::'            the single-learner kernels
  --match 'her_sample|index_episodes'    the trajectory store's kernels"""
import argparse
import collections
import re
import sys

import isa

LANE_KERNELS = r"^env_(step|rollout|rollout_async|reset|summary)_kernel<"
RESOURCES = ("vgpr", "agpr", "sgpr", "scratch", "lds", "spill_vgpr")


def kernels(lib, match):
    """{demangled name without return type and arguments: (metadata, [Inst] up to the last s_endpgm)}; what follows that is the
    padding between kernels and after the last one"""
    out = {}
    for _, dm, md, ins in isa.all_kernels(lib):
        if match and not re.search(match, dm):
            continue
        ends = [k for k, i in enumerate(ins) if i.mnem == "s_endpgm"]
        out[_name(dm)] = (md, ins[:ends[-1] + 1] if ends else ins)
    return out


def _name(demangled):
    """the kernel's name with its template arguments: the return type goes, and the parameter list -- the parenthesis that the
    signature's last one closes, so a parameter type with parentheses of its own does not cut the name short"""
    s = re.sub(r"^void ", "", demangled)
    if not s.endswith(")"):
        return s
    depth = 0
    for k in range(len(s) - 1, -1, -1):
        depth += (s[k] == ")") - (s[k] == "(")
        if depth == 0:
            return s[:k]
    return s


def _res(md):
    return " ".join("%s %d" % (k, md[k]) for k in RESOURCES)


def _loops(ins):
    return [isa.mix(ins[a:b + 1]) for a, b in isa.innermost_loops(ins)]


def _loop_changes(l0, l1):
    """the loops whose mix moved, as 'loop k: class a -> b, ...'"""
    if len(l0) != len(l1):
        return ["%d loops -> %d loops" % (len(l0), len(l1))]
    return ["loop %d: " % k + ", ".join("%s %d -> %d" % (c, x.get(c, 0), y.get(c, 0)) for c in sorted(set(x) | set(y)) if x.get(c, 0) != y.get(c, 0))
            for k, (x, y) in enumerate(zip(l0, l1)) if x != y]


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--match", default=None)
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=isa.LIB)
    a = ap.parse_args(argv)
    old, new = kernels(a.old, a.match), kernels(a.new, a.match)
    fam = collections.defaultdict(lambda: collections.defaultdict(list))     # family -> state -> [(delta, resource went up, loops moved)]
    bad = 0
    for name in sorted(set(old) | set(new)):
        lane = re.search(LANE_KERNELS, name) is not None
        family = name.split("<")[0]
        if name not in old or name not in new:
            state = "new" if name not in old else "MISSING"
            md, ins = (new if name in new else old)[name]
            print("%-12s %s\n    %d instructions, %s" % (state, name, len(ins), _res(md)))
            bad += state == "MISSING" and not lane
            fam[family][state].append((0, False, False))
            continue
        (md0, i0), (md1, i1) = old[name], new[name]
        t0, t1 = [i.text for i in i0], [i.text for i in i1]
        if t0 == t1 and md0 == md1:
            state = "identical"
        elif collections.Counter(i.mnem for i in i0) == collections.Counter(i.mnem for i in i1):
            state = "re-allocated"
        else:
            state = "DIFFERENT"
        bad += state != "identical" and not lane
        print("%-12s %s%s" % (state, name, "" if state == "identical" or lane else "   <-- not a lane kernel"))
        if state == "identical":
            print("    %d instructions, %s" % (len(t1), _res(md1)))
            fam[family][state].append((0, False, False))
            continue
        first = next((k for k, (x, y) in enumerate(zip(t0, t1)) if x != y), min(len(t0), len(t1)))
        print("    instructions %d -> %d (%+d), first difference at %d" % (len(t0), len(t1), len(t1) - len(t0), first))
        print("    old: %s\n    new: %s" % (_res(md0), _res(md1)))
        up = [k for k in RESOURCES if md1[k] > md0[k]]
        if up:
            print("    higher: " + ", ".join("%s %d -> %d" % (k, md0[k], md1[k]) for k in up))
        moved = _loop_changes(_loops(i0), _loops(i1))
        print("    innermost loops: " + ("same instruction mix" if not moved else "MIX MOVED: " + "; ".join(moved)))
        fam[family][state].append((len(t1) - len(t0), bool(set(up) - {"sgpr"}), bool(moved)))
    print("\nfamily: kernels by state [instruction delta min .. max; with vgpr / agpr / scratch / lds / spills higher; with a loop mix moved]")
    for family in sorted(fam):
        parts = []
        for state, rows in sorted(fam[family].items()):
            d = [r[0] for r in rows]
            parts.append("%d %s" % (len(rows), state) + ("" if state in ("identical", "new", "MISSING") else
                         " [%+d .. %+d; %d; %d]" % (min(d), max(d), sum(r[1] for r in rows), sum(r[2] for r in rows))))
        print("  %s: %s" % (family, ", ".join(parts)))
    print("%d kernels outside the lane families differ or are missing" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
