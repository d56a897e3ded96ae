#!/usr/bin/env python3
"""Milliseconds per step of the population trajectory store (armenv.replay.PopulationTrajectoryStore: ONE armenv_her_pop_sample per
batch of P members; ONE add_rollouts + ready() per iteration) against the path it replaces, member by member:

  sample   one PopulationTrajectoryStore.sample(out=stacked batch)   vs   P TrajectoryStore.sample(out=member p's slice)
           at (P, B) in {(4, 256), (16, 256), (64, 256), (16, 2048)}, rings of N = 64 envs x 1536 steps, full
  add      one add_rollouts + ready(5)                               vs   P (add_rollout + size())
           at (P, N, steps, cap) = (16, 64, 32, 1536)

The member stores of the sample legs read the population store's own rings (member_view), so both legs gather the same data.  One
process, warmed up, five repeats with the legs alternating; each repeat is one pair of HIP events around 30 steps (the span on the
device, launch gaps included -- a step here IS mostly launches).  Medians, and the ratio from the medians and from the extreme repeats.

    python tests/tools/time_pop_store.py [--out profiles/pop_store_time.json]
    python tests/tools/time_pop_store.py --only population --what sample --cases 16x256      # one leg alone (for rocprofv3 --stats)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "drl-on-robot-arm_amd")]
import torch  # noqa: E402

from armenv.replay import PopulationTrajectoryStore, TrajectoryStore  # noqa: E402

LEGS = ("population", "members")
DEV = "cuda:0"


def _fill_staging(store, gen, P, steps, N, D):
    bufs = store.rollout_buffers(steps, N, D)
    for k, t in store._staging.items():
        r = torch.rand(t.shape, device=DEV, generator=gen)
        t.copy_((r < 0.05) if t.dtype == torch.uint8 else r)          # episodes of about 20 steps
    return bufs


def _filled_store(gen, P, N, D, cap, chunk=32):
    """a population store whose rings are full (cap steps, added in chunks of `chunk`)"""
    store = PopulationTrajectoryStore(P, device=DEV, seed=0, capacity_steps=cap)
    obs0 = torch.rand(P, N, D, device=DEV, generator=gen)
    for it in range(cap // chunk + 1):
        _fill_staging(store, gen, P, chunk, N, D)
        store.add_rollouts(obs0, starts_at_reset=(it == 0))
    return store, obs0


def _batch(P, B, D):
    return dict(states=torch.zeros(P, B, D, device=DEV), actions=torch.zeros(P, B, 3, device=DEV), next_states=torch.zeros(P, B, D, device=DEV),
                rewards=torch.zeros(P, B, device=DEV), dones=torch.zeros(P, B, dtype=torch.uint8, device=DEV))


def _sample_legs(gen, P, B, only):
    store, _ = _filled_store(gen, P, 64, 6, 1536)
    batch = _batch(P, B, 6)
    step = {}
    if only in (None, "population"):
        step["population"] = lambda: store.sample(B, use_her=True, her_ratio=0.8, out=batch)
    if only in (None, "members"):
        singles = []
        for p in range(P):
            s = TrajectoryStore(device=DEV, seed=p)
            s.chunk = store.member_view(p)
            singles.append((s, {k: t[p] for k, t in batch.items()}))

        def members():
            for s, out in singles:
                s.sample(B, use_her=True, her_ratio=0.8, out=out)
        step["members"] = members
    return step, min(store.sizes())


def _add_legs(gen, P, N, steps, cap, only):
    step = {}
    store, obs0 = _filled_store(gen, P, N, 6, cap, chunk=steps)
    bufs = _fill_staging(store, gen, P, steps, N, 6)
    if only in (None, "population"):
        def population():
            store.add_rollouts(obs0, starts_at_reset=False)
            store.ready(5)
        step["population"] = population
    if only in (None, "members"):
        singles = [TrajectoryStore(device=DEV, seed=p, capacity_steps=cap) for p in range(P)]
        for it in range(cap // steps + 1):
            for p, s in enumerate(singles):
                s.add_rollout(obs0[p], bufs[p], starts_at_reset=(it == 0))

        def members():
            for p, s in enumerate(singles):
                s.add_rollout(obs0[p], bufs[p], starts_at_reset=False)
                s.size()
        step["members"] = members
    return step, min(store.sizes())


def _time(step, steps, repeats):
    for fn in step.values():                     # warm-up: allocations, code objects, clocks
        for _ in range(12):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in step}                # ms per step of the leg
    for _ in range(repeats):
        for name, fn in step.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sample,add")
    ap.add_argument("--cases", default="4x256,16x256,64x256,16x2048", help="PxB of the sample legs, comma separated")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=LEGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    work = []
    if "sample" in a.what.split(","):
        work += [("sample", dict(members=P, batch=B, envs=64, cap=1536), lambda P=P, B=B: _sample_legs(gen, P, B, a.only))
                 for P, B in [tuple(int(x) for x in c.split("x")) for c in a.cases.split(",")]]
    if "add" in a.what.split(","):
        work.append(("add", dict(members=16, envs=64, steps=32, cap=1536), lambda: _add_legs(gen, 16, 64, 32, 1536, a.only)))
    rows = []
    for what, shape, make in work:
        step, fewest = make()
        times = _time(step, a.steps, a.repeats)
        for name, ts in times.items():
            rec = dict(what=what, **shape, leg=name, ms_per_step=round(statistics.median(ts), 4), ms_min=round(min(ts), 4),
                       ms_max=round(max(ts), 4), spread=round((max(ts) - min(ts)) / statistics.median(ts), 4),
                       fewest_episodes_of_a_member=fewest, repeats=a.repeats, steps_per_repeat=a.steps, clock="HIP events")
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        if len(times) == 2:
            x, y = times["members"], times["population"]
            rec = dict(what=what, **shape, speedup_of="population", over="members", ratio=round(statistics.median(x) / statistics.median(y), 3),
                       ratio_min=round(min(x) / max(y), 3), ratio_max=round(max(x) / min(y), 3))
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        del step
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
