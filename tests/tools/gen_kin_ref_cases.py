#!/usr/bin/env python3
"""Writes tests/golden/kin_ref_cases.npz: the case table of tests/kin_cases.py with the 40-digit reference values and the derived bounds
of tests/kin_ref.py (CPU only, needs mpmath; about a minute).  tests/test_kin_ref.py regenerates the table and compares array for array."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "drl-on-robot-arm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import kin_cases
    T = kin_cases.build()
    out = os.path.join(ROOT, "tests", "golden", "kin_ref_cases.npz")
    np.savez_compressed(out, **T)
    n_fk = sum(len(T[k]) for k in T if k.startswith("fk.") and k.endswith(".q"))
    n_ik = sum(len(T[k]) for k in T if k.startswith("ik.") and k.endswith(".q"))
    print(f"{out}: {n_fk} FK poses, {n_ik} IK cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
