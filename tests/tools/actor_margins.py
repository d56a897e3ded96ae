#!/usr/bin/env python3
"""How much slack the derived forward bounds of tests/actor_ref64.py have: one run on the GPU over every case of
tests/actor_cases.py writes max(err / bound) per case and per kernel (exact-f32 actor, f16x3 actor, the four-net take_action pass:
q1, q2, picked action) as JSON.  No test depends on these figures.

    python tests/tools/actor_margins.py [--out profiles/actor_ref64_margins.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "drl-on-robot-arm_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import actor_cases as K  # noqa: E402
import actor_ref64 as R  # noqa: E402
import actor_ref64_gpu as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_ref64_margins.json"))
    args = ap.parse_args()
    handles = {D: G.handle(D) for D in (6, 9)}
    cases = {}
    for c in K.SINGLE:
        s = K.single(c["id"])
        row = {}
        for kind, b in (("actor", s["b32"]), ("actor_f16x3", s["b16"])):
            row[kind] = G.ratio(G.single_forward(handles[c["D"]], kind, s["net"], s["x"], s["bound"]), s["ref"]["out"], b["out"])
        cases[c["id"]] = row
    for c in K.FOUR:
        f = K.four(c["id"])
        r, ok = G.four_ok(G.four_forward(handles[c["D"]], c["agent"], f["nets"], f["x"], f["bound"]), f["b"])
        cases[c["id"]] = dict(datd3_forward=dict(q1=r["q1"], q2=r["q2"], action=r["action"], picks_agree=r["picks_agree"]))
    for e in handles.values():
        e.close()
    worst = {k: max(row[k] for row in cases.values() if k in row) for k in ("actor", "actor_f16x3")}
    worst["datd3_forward"] = max(max(v["datd3_forward"][k] for k in ("q1", "q2", "action")) for v in cases.values() if "datd3_forward" in v)
    out = dict(what="max |kernel - float64| / derived bound (tests/actor_ref64.py), per case of tests/actor_cases.py and per kernel",
               rows_per_case=K.N, tanhf_ulp_assumed=R.TANHF_ULP, largest=worst, cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(worst))


if __name__ == "__main__":
    main()
