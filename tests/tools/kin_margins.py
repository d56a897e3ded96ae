#!/usr/bin/env python3
"""Runs the GPU comparisons of tests/test_gpu_kin_ref.py once and writes the largest err / bound per (kernel path, family, precision)
to profiles/kin_ref_margins.json.  Measured values, written down after the run: nothing in the tests is tuned to them.  A ratio above 1
is a finding (the derivation is wrong, or the kernel is); a family whose ratios are all below ~1e-3 is one where a defect can hide."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "drl-on-robot-arm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import kin_fixture as KF
    import kin_ref_gpu as G
    from armenv import envs
    T = KF.load()
    out = {}

    def put(path, prec, fam, ratios, use=None):
        for f, v in KF.worst_by_family(T, fam, ratios, use).items():
            k = f"{path}|{f}|f{prec}"
            out[k] = max(out.get(k, 0.0), v)
    for path in KF.CHAIN_PATHS:
        for prec in (64, 32):
            fam = T[f"fk.{path}.family"]
            for idx, pos, quat in G.run_fk(envs, T, path, prec):
                rp, rq, use = KF.fk_ratios(T, path, prec, pos, quat, idx)      # (the families an engine is not compared on: no entry)
                put(f"armenv_fk:{path}:pos", prec, fam[idx], rp, use)
                put(f"armenv_fk:{path}:quat", prec, fam[idx], rq, use)
    for name in [str(s) for s in T["ik_groups"]]:
        fam = T[f"ik.{name}.family"]
        for prec in T[f"ik.{name}.precs"].tolist():
            if name.startswith("step"):
                for idx in G.batches(len(fam)):
                    for kern, (q, trig) in G.run_step(envs, T, name, prec, idx).items():
                        r, rt = KF.ik_ratios(T, name, prec, q, trig, idx)
                        put(f"{kern}_kernel:{name}:q", prec, fam[idx], r)
                        put(f"{kern}_kernel:{name}:pair", prec, fam[idx], rt)
                continue
            runs, (q_rep, _) = G.run_ik(envs, T, name, prec)
            for idx, qo, _ in runs:
                put(f"armenv_ik:{name}", prec, fam[idx], KF.ik_ratios(T, name, prec, qo, idx=idx)[0])
            put(f"armenv_ik:{name}:alone_in_wave", prec, fam, KF.ik_ratios(T, name, prec, q_rep[:, 0])[0])
    for task in ("reach", "push", "pick"):
        for prec in (64, 32):
            d = G.run_drift(envs, task, prec)
            out[f"drift:{task}:pair|511_steps|f{prec}"] = float((d["pair_err"] / d["bound"]).max())
            out[f"drift:{task}:norm|511_steps|f{prec}"] = float((d["norm_err"] / (2 * np.sqrt(2) * d["bound"])).max())
    dst = os.environ.get("KIN_MARGINS_OUT", os.path.join(ROOT, "profiles", "kin_ref_margins.json"))
    with open(dst, "w") as fh:
        json.dump({"what": "largest err / derived bound per kernel path | family | precision (tests/tools/kin_margins.py)",
                   "ratios": {k: float("%.4g" % v) for k, v in sorted(out.items())}}, fh, indent=1)
        fh.write("\n")
    worst = max(out.items(), key=lambda kv: kv[1])
    print("wrote", dst, "largest ratio", worst)


if __name__ == "__main__":
    main()
