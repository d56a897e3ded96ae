#!/usr/bin/env python3
"""The two records of the shared population sampler (PopulationTrajectoryStore.sample(share_ratio=...), armenv_her_pop_sample_shared;
armenv.train_pop --share-replay).  Neither has a pass bar: they are measured and reported as found.

  time   microseconds per call, on the HOST clock (perf_counter around 200 calls and one synchronise: a launch of this size is
         mostly its Python call, so this is what a training loop pays), of
             own          sample(out=batch)                       armenv_her_pop_sample, the path of a run without sharing
             shared 0.5   sample(out=batch, share_ratio=0.5)      armenv_her_pop_sample_shared
             shared 1.0   sample(out=batch, share_ratio=1.0)
         at P = 16 and 64, B = 256, D = 6, rings of 64 envs x 1536 steps, full.  One process, warmed up, five repeats with the
         legs alternating; medians and extremes.
  ab     python -m armenv.train_pop --members 8 --iterations 100 [--pbt-every 10] --share-replay R --seed S on reach (the
         function behind the command, called in this process) for R in 0, 0.5, 1 and S in 0, 1, 2: per member the first LOGGED
         iteration (every 10th) whose success rate since the last record reaches 90 %, or null; the last record's rates.

    python tests/tools/pop_shared_replay.py --what time --out profiles/pop_shared_sample_time.json
    python tests/tools/pop_shared_replay.py --what ab --out profiles/pop_shared_replay_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "drl-on-robot-arm_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from time_pop_store import DEV, _batch, _filled_store  # noqa: E402

RATIOS = (0.0, 0.5, 1.0)


def time_sample(members, calls, repeats, B=256, D=6, envs=64, cap=1536):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    rows = []
    for P in members:
        store, _ = _filled_store(gen, P, envs, D, cap)
        batch = _batch(P, B, D)
        legs = {"own": lambda: store.sample(B, use_her=True, her_ratio=0.8, out=batch)}
        for ratio in RATIOS[1:]:
            legs["shared %.1f" % ratio] = lambda ratio=ratio: store.sample(B, use_her=True, her_ratio=0.8, out=batch, share_ratio=ratio)
        for fn in legs.values():                 # warm-up: the kept argument structs are rebuilt when the ratio changes; code objects
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for name, fn in legs.items():
                fn()                             # the struct of this leg
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / calls * 1e6)
        for name, ts in times.items():
            rec = dict(what="sample", members=P, batch=B, obs_dim=D, envs=envs, cap=cap, leg=name, us_per_call=round(statistics.median(ts), 2),
                       us_min=round(min(ts), 2), us_max=round(max(ts), 2), repeats=repeats, calls_per_repeat=calls,
                       fewest_episodes_of_a_member=min(store.sizes()), clock="host perf_counter, one synchronise per repeat")
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        del store, batch, legs
        torch.cuda.empty_cache()
    return rows


def first_reaching(history, members, bar=0.9):
    first = [None] * members
    for rec in history:
        if rec.get("kind") is None:
            for p, rate in enumerate(rec["success_rate"]):
                if first[p] is None and rate >= bar:
                    first[p] = rec["iteration"]
    return first


def ab(members, iterations, seeds):
    from armenv.train_pop import train_reach_population
    rows = []
    for pbt_every in (None, 10):
        for seed in seeds:
            for ratio in RATIOS:
                pbt = None if pbt_every is None else dict(every=pbt_every)
                _, history = train_reach_population(members=members, iterations=iterations, seed=seed, share_ratio=ratio, pbt=pbt,
                                                    device=DEV, log=lambda line: None)
                logged = [rec for rec in history if rec.get("kind") is None]
                replaced = sum(len(rec["new"]) for rec in history if rec.get("kind") == "pbt")
                command = "python -m armenv.train_pop --members %d --iterations %d --seed %d --share-replay %g" % (members, iterations, seed, ratio)
                rec = dict(what="ab", command=command + ("" if pbt_every is None else " --pbt-every %d" % pbt_every), pbt_every=pbt_every,
                           seed=seed, share_ratio=ratio, first_iteration_with_success_90=first_reaching(history, members),
                           last_success_rate=[round(r, 4) for r in logged[-1]["success_rate"]],
                           mean_success_rate_by_record=[round(statistics.mean(r["success_rate"]), 4) for r in logged],
                           members_replaced=replaced, wall_s=round(logged[-1]["wall_s"], 2))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="time", choices=["time", "ab"])
    ap.add_argument("--members", default=None, help="time: comma separated (16,64); ab: one number (8)")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "time":
        rows = time_sample([int(x) for x in (a.members or "16,64").split(",")], a.calls, a.repeats)
    else:
        rows = ab(int(a.members or 8), a.iterations, [int(x) for x in a.seeds.split(",")])
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
