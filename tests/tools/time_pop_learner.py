#!/usr/bin/env python3
"""Milliseconds per population step of the fused DADDPG, DATD3 and DARC population updates (armenv_daddpg_pop_update,
armenv_datd3_pop_update: ONE update of P members) against the path they replace, P sequential single-learner calls
(FusedDADDPG.train; FusedDATD3 / FusedDARC.update, one learner each), at (P, B) in {(4, 256), (16, 256), (64, 256), (16, 2048)}.
A step is ONE update of every member (for DATD3 / DARC: k alternating 1, 2, so two steps are one `train`).  One process, warmed up,
five repeats with the legs alternating, each repeat a device-synchronised host clock around 30 steps; medians, and the speed-up from
the medians and from the extreme repeats (spread).  The protocol of time_td3_pop_learner.py.

    python tests/tools/time_pop_learner.py [--out profiles/pop2_time_learner.json] [--agents daddpg,datd3,darc] [--cases 16x256,...]
    python tests/tools/time_pop_learner.py --only population --agents daddpg --cases 16x256      # one leg alone (for rocprofv3 --stats)
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

from armenv.fused_daddpg import FusedDADDPG  # noqa: E402
from armenv.fused_daddpg_pop import FusedDADDPGPopulation  # noqa: E402
from armenv.fused_datd3 import FusedDARC, FusedDATD3  # noqa: E402
from armenv.fused_datd3_pop import FusedDARCPopulation, FusedDATD3Population  # noqa: E402

LEGS = ("population", "sequential")
AGENTS = dict(daddpg=(FusedDADDPGPopulation, FusedDADDPG), datd3=(FusedDATD3Population, FusedDATD3), darc=(FusedDARCPopulation, FusedDARC))


def _batch(gen, dev, *lead):
    r = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    return dict(states=r(*lead, 6), actions=r(*lead, 3) - 0.5, next_states=r(*lead, 6), rewards=r(*lead),
                dones=(r(*lead) < 0.1).to(torch.uint8))


def _stepper(agent, learner, batch):
    """one update of `learner` (a population or a single learner) per call"""
    if agent == "daddpg":
        return lambda: learner.train(batch)
    return lambda: learner.update(batch, update_a1=learner.total_it % 2 == 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default="daddpg,datd3,darc")
    ap.add_argument("--cases", default="4x256,16x256,64x256,16x2048", help="PxB, comma separated")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=LEGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    rows = []
    for agent in a.agents.split(","):
        Pop, Single = AGENTS[agent]
        for P, B in [tuple(int(x) for x in c.split("x")) for c in a.cases.split(",")]:
            gen = torch.Generator(device=dev)
            gen.manual_seed(1)
            stacked = _batch(gen, dev, P, B)
            step = {}
            if a.only in (None, "population"):
                step["population"] = _stepper(agent, Pop(P, 6, 3, 0.7, device=dev), stacked)
            if a.only in (None, "sequential"):
                kw = [{} if agent == "daddpg" else dict(seed=p) for p in range(P)]
                singles = [_stepper(agent, Single(6, 3, 0.7, device=dev, **kw[p]), {k: v[p] for k, v in stacked.items()}) for p in range(P)]

                def sequential(singles=singles):
                    for f in singles:
                        f()
                step["sequential"] = sequential
            for fn in step.values():                 # warm-up: allocations, code objects, clocks
                for _ in range(12):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in step}            # ms per step of the leg
            for _ in range(a.repeats):
                for name, fn in step.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
            for name, ts in times.items():
                rec = dict(agent=agent, members=P, batch=B, leg=name, ms_per_step=round(statistics.median(ts), 4), ms_min=round(min(ts), 4),
                           ms_max=round(max(ts), 4), spread=round((max(ts) - min(ts)) / statistics.median(ts), 4),
                           updates_per_step=P, repeats=a.repeats, steps_per_repeat=a.steps)
                rows.append(rec)
                print(json.dumps(rec), flush=True)
            if "population" in times and "sequential" in times:
                x, y = times["sequential"], times["population"]
                rec = dict(agent=agent, members=P, batch=B, speedup_of="population", over="sequential",
                           ratio=round(statistics.median(x) / statistics.median(y), 3), ratio_min=round(min(x) / max(y), 3),
                           ratio_max=round(max(x) / min(y), 3))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
            del step
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
