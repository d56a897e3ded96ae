#!/usr/bin/env python3
"""Milliseconds per DADDPG update at B in {256, 2048, 8192}: the torch learner issued eagerly (DADDPG.train), the torch learner
replayed from its hipGraphs (DADDPG.train_graphed) and the fused HIP update (FusedDADDPG.train), in one process, warmed up, five
repeats with the three learners alternating, each repeat a device-synchronised host clock around 30 updates (both actors' updates
alternate inside every repeat).  Prints one JSON line per (B, learner) with the median and the spread, the FLOP of an update counted
from the shapes and the share of the f32 matrix peak that is.  The protocol of time_learner.py (the TD3 update's timer).

    python tests/tools/time_daddpg_learner.py [--out profiles/daddpg_fused_time_learner.json] [--batches 256,2048,8192]
    python tests/tools/time_daddpg_learner.py --fused-only --batches 2048     # the fused update alone (for rocprofv3 --stats)
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

from armenv.daddpg import DADDPG  # noqa: E402
from armenv.fused_daddpg import FusedDADDPG  # noqa: E402

F32_MATRIX_PEAK = 157.3e12     # MI355X, v_mfma_f32_*: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def flop_per_update(B, D, H=256, A=3):
    """forward 2 B in out per linear; backward 2 B in out for the input delta where one is needed, 2 B in out for the weights.
    Every DADDPG update steps the critic and one actor."""
    K1 = D + A
    lin = lambda i, o: 2 * B * i * o
    mlp = lambda i, o: lin(i, H) + lin(H, H) + lin(H, o)
    critic = (2 * mlp(D, A) + 2 * mlp(K1, 1)    # both target actors, the target critic over both proposals
              + mlp(K1, 1)                      # critic forward
              + lin(H, 1) + lin(H, H)           # critic backward: input deltas of layers 3 and 2
              + mlp(K1, 1))                     # critic weight gradients
    actor = (mlp(D, A) + mlp(K1, 1)             # actor k, stepped critic forward
             + lin(H, 1) + lin(H, H) + lin(K1, H)   # critic backward to the action
             + lin(H, A) + lin(H, H)            # actor input deltas of layers 3 and 2
             + mlp(D, A))                       # actor weight gradients
    return critic + actor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,2048,8192")
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        torch.manual_seed(0)
        learners = {"fused": FusedDADDPG(6, 3, 0.7, device=dev)}
        if not a.fused_only:
            learners["torch_eager"] = DADDPG(6, 3, 0.7, device=dev)
            learners["torch_graphed"] = DADDPG(6, 3, 0.7, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        batch = dict(states=torch.rand(B, 6, device=dev, generator=gen), actions=torch.rand(B, 3, device=dev, generator=gen) - 0.5,
                     next_states=torch.rand(B, 6, device=dev, generator=gen), rewards=torch.rand(B, device=dev, generator=gen),
                     dones=(torch.rand(B, device=dev, generator=gen) < 0.1).to(torch.uint8))
        fused_in = learners["fused"].batch_buffers(B)
        for k, v in fused_in.items():
            v.copy_(batch[k])
        step = {"fused": lambda: learners["fused"].train(fused_in)}
        if not a.fused_only:
            static = learners["torch_graphed"].capture(B)
            for k, v in static.items():
                v.copy_(batch[k])
            step["torch_eager"] = lambda: learners["torch_eager"].train(batch)
            step["torch_graphed"] = lambda: learners["torch_graphed"].train_graphed(static)
        for name, fn in step.items():            # warm-up: allocations, optimiser state, code objects, clocks
            for _ in range(12):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in step}
        for _ in range(a.repeats):
            for name, fn in step.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.updates):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / a.updates)
        fl = flop_per_update(B, 6)
        for name, ts in times.items():
            med = statistics.median(ts)
            rec = dict(batch=B, learner=name, ms_per_update=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                       repeats=a.repeats, updates_per_repeat=a.updates, gflop_per_update=round(fl / 1e9, 4),
                       tflops=round(fl / (med * 1e-3) / 1e12, 3), share_of_f32_matrix_peak=round(fl / (med * 1e-3) / F32_MATRIX_PEAK, 5))
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        for name in ("torch_graphed", "torch_eager"):
            if name in times:
                r = statistics.median(times["fused"]) / statistics.median(times[name])
                rec = dict(batch=B, fused_over=name, ratio=round(r, 3))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
        del learners, step
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
