#!/usr/bin/env python3
"""Milliseconds per update of the population updates through the per-member entry points (armenv_*_pop_update_hyper) against the
shared-scalar ones (armenv_*_pop_update), for TD3, DADDPG, DATD3 and DARC at P = 16, B = 256, D = 6.  Three legs in one process:
  shared         the population as it always was: armenv_*_pop_update
  hyper_same     the per-member entry point with every member holding the shared values (``always_hyper``): the same bits
  hyper_swept    the per-member entry point with P different learning rates, discounts, Polyak rates (and noise scales, DARC weights)
An update is one call of every member (DATD3 / DARC: k alternating 1, 2).  Warmed up, then `--repeats` rounds with the legs
alternating, each a device-synchronised host clock around `--steps` updates; medians and the spread (max - min) / median per leg, and
the ratio of the medians.  Before timing, `shared` and `hyper_same` are checked to have trained the same bits.

    python tests/tools/time_pop_hyper.py [--out profiles/pop_hyper_time_learner.json] [--agents td3,daddpg,datd3,darc]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "drl-on-robot-arm_amd")]
import torch  # noqa: E402

from armenv.train_pop import _POPULATIONS  # noqa: E402

LEGS = ("shared", "hyper_same", "hyper_swept")


def _batch(gen, dev, *lead):
    r = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    return dict(states=r(*lead, 6), actions=r(*lead, 3) - 0.5, next_states=r(*lead, 6), rewards=r(*lead),
                dones=(r(*lead) < 0.1).to(torch.uint8))


def _stepper(agent, pop, batch):
    if agent in ("td3", "daddpg"):
        return lambda: pop.train(batch)
    return lambda: pop.update(batch, update_a1=pop.total_it % 2 == 0)


def _swept(Pop, P):
    """P different values of every sweepable name, inside the usual ranges"""
    ramp = lambda lo, hi: [lo + (hi - lo) * p / max(1, P - 1) for p in range(P)]
    ranges = dict(actor_lr=(1e-4, 2e-3), critic_lr=(2e-3, 1e-4), tau=(0.001, 0.02), gamma=(0.9, 0.995), policy_noise=(0.1, 0.3),
                  noise_clip=(0.3, 0.6), q_weight=(0.1, 0.9), regularization_weight=(0.001, 0.02))
    return {n: ramp(*ranges[n]) for n in Pop.sweepable()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default="td3,daddpg,datd3,darc")
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, P, B = "cuda:0", a.members, a.batch
    rows = []
    for agent in a.agents.split(","):
        Pop = _POPULATIONS[agent]
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        stacked = _batch(gen, dev, P, B)
        pops = dict(shared=Pop(P, 6, 3, 0.7, device=dev), hyper_same=Pop(P, 6, 3, 0.7, device=dev),
                    hyper_swept=Pop(P, 6, 3, 0.7, device=dev, **_swept(Pop, P)))
        pops["hyper_same"].always_hyper = True
        assert [pops[k].entry_point.endswith("_hyper") for k in LEGS] == [False, True, True]
        step = {k: _stepper(agent, pops[k], stacked) for k in LEGS}
        for fn in step.values():                 # warm-up: allocations, code objects, clocks
            for _ in range(12):
                fn()
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for p in range(P) for x, y in zip(pops["shared"]._member_state(p), pops["hyper_same"]._member_state(p)))
        assert same, "%s: the per-member entry point with shared values trained other bits than the shared one" % agent
        times = {k: [] for k in LEGS}
        for _ in range(a.repeats):
            for name, fn in step.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for name, ts in times.items():
            rec = dict(agent=agent, members=P, batch=B, leg=name, entry_point=pops[name].entry_point,
                       ms_per_update=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                       spread=round((max(ts) - min(ts)) / statistics.median(ts), 4), repeats=a.repeats, steps_per_repeat=a.steps,
                       same_bits_as_shared=same if name == "hyper_same" else None)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        for name in LEGS[1:]:
            rec = dict(agent=agent, members=P, batch=B, ratio_of=name, over="shared",
                       ratio=round(statistics.median(times[name]) / statistics.median(times["shared"]), 4),
                       ratio_min=round(min(times[name]) / max(times["shared"]), 4), ratio_max=round(max(times[name]) / min(times["shared"]), 4))
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        del step, pops
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
